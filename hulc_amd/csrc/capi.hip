// hulc_amd/csrc/capi.hip — extern "C" boundary of libhulc_hip.so (see include/hulc_hip.h).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <stdexcept>

#include "engine.h"
#include "sbert.h"
#include "store_gather.h"
#include "store_stage.h"

using namespace hulc_bf16;      // this translation unit: fp32 (parity) + bf16 engines and the per-kernel test entry points; fp16: engine_f16.hip

static thread_local char g_err[1024] = "";
void hulc_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct hulc_ctx {
    IEngine* e = nullptr;
    StoreStager stager;      // host tier of a two-tier frame store (store_stage.h); its stream and events are created by the first hulc_store_stage
};

extern "C" {

const char* hulc_last_error(void) { return g_err; }

int hulc_ctx_create(const hulc_config* cfg, hulc_ctx** out) {
    if (!cfg || !out) { hulc_set_error("hulc_ctx_create: null argument"); return 1; }
    if (cfg->max_seq > 64 || cfg->max_seq < 1 || cfg->max_batch < 1 || cfg->max_window < cfg->max_seq) {
        hulc_set_error("hulc_ctx_create: need 1 <= max_seq <= 64, max_batch >= 1, max_window >= max_seq");
        return 1;
    }
    // every dropout site divides by 1 - p (the fused transformer kernels among them): p = 1, p > 1 or NaN would reach the kernels as inf / NaN multipliers
    if (!(cfg->dropout_p >= 0.f && cfg->dropout_p < 1.f)) { hulc_set_error("hulc_ctx_create: dropout_p=%g must be in [0, 1)", (double)cfg->dropout_p); return 1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { hulc_set_error("hulc_ctx_create: no HIP device visible"); return 1; }
    hulc_ctx* c = new hulc_ctx();
    int rc = 1;
    if (cfg->dtype == HULC_DTYPE_F32 || cfg->dtype == HULC_DTYPE_BF16) c->e = hulc_bf16::make_engine(*cfg, &rc);
    else if (cfg->dtype == HULC_DTYPE_F16) c->e = hulc_f16::make_engine(*cfg, &rc);
    else { hulc_set_error("hulc_ctx_create: unknown dtype %d", cfg->dtype); delete c; return 1; }
    if (rc) { delete c->e; delete c; return rc; }
    *out = c;
    return 0;
}
int hulc_ctx_destroy(hulc_ctx* ctx) {
    if (!ctx) return 0;
    hipDeviceSynchronize();
    delete ctx->e;
    delete ctx;
    return 0;
}
int hulc_set_stream(hulc_ctx* ctx, void* s) { ctx->e->st = (hipStream_t)s; return 0; }
int64_t hulc_workspace_bytes(const hulc_ctx* ctx) { return ctx->e->workspace_bytes(); }
int hulc_bind_params(hulc_ctx* ctx, float* p, float* g, float* m, float* v, int64_t numel, int32_t n, const char* const* names, const int64_t* offs,
                     const int64_t* numels) {
    if (!ctx || !p || !g || !m || !v) { hulc_set_error("hulc_bind_params: null argument"); return 1; }
    return ctx->e->bind(p, g, m, v, numel, n, names, offs, numels);
}
int hulc_prepare_weights(hulc_ctx* ctx) { return ctx->e->prepare_weights(); }
int hulc_zero_grads(hulc_ctx* ctx) { return ctx->e->zero_grads(); }
int hulc_flush_grads(hulc_ctx* ctx) { return ctx->e->flush_grads(); }
int hulc_forward_loss(hulc_ctx* ctx, const hulc_batch* b, float lw, float cw, float* out, int32_t on_host) {
    if (!ctx || !b) { hulc_set_error("hulc_forward_loss: null argument"); return 1; }
    return ctx->e->forward(b, lw, cw, out, on_host);
}
int hulc_forward_loss_pair(hulc_ctx* ctx, const hulc_batch* v, const hulc_batch* l, float lw, float cw, float* out, int32_t on_host) {
    if (!ctx || !v || !l) { hulc_set_error("hulc_forward_loss_pair: null argument"); return 1; }
    return ctx->e->forward_pair(v, l, lw, cw, out, on_host);
}
int hulc_backward(hulc_ctx* ctx) { return ctx->e->backward(-1); }
int hulc_backward_part(hulc_ctx* ctx, int32_t part) {
    if (part != 0 && part != 1) { hulc_set_error("hulc_backward_part: part must be 0 or 1"); return 1; }
    return ctx->e->backward(part);
}
int hulc_validate(hulc_ctx* ctx, const hulc_batch* batch, const hulc_val_noise* noise, float* out_host, int32_t* plan_idx_pp_out, int32_t* plan_idx_pr_out,
                  float* pred_pp_out, float* pred_pr_out) {
    if (!batch) { hulc_set_error("hulc_validate: null batch"); return 1; }
    return ctx->e->validate(batch, noise, out_host, plan_idx_pp_out, plan_idx_pr_out, pred_pp_out, pred_pr_out);
}
int hulc_store_gather(hulc_ctx* ctx, const hulc_store_tables* t, const int64_t* window_start, const int32_t* window_len, const int32_t* lang_row, int32_t B, int32_t S,
                      float* actions_out, float* robot_obs_out, float* lang_out) {
    if (!ctx || !t || !window_start || !actions_out || !robot_obs_out) { hulc_set_error("hulc_store_gather: null argument"); return 1; }
    if (!t->actions || !t->robot_obs || t->store_frames < 1) { hulc_set_error("hulc_store_gather: needs the actions and robot_obs tables and store_frames >= 1 (got %lld)", (long long)t->store_frames); return 1; }
    if (B < 1 || S < 1 || (long long)B * S * 22 + (long long)B * 384 > 0x7fffffffll) { hulc_set_error("hulc_store_gather: bad shape B=%d S=%d", B, S); return 1; }
    if (lang_out && (!t->lang || !lang_row || t->lang_rows < 1)) { hulc_set_error("hulc_store_gather: lang_out needs the lang table (lang_rows >= 1) and lang_row"); return 1; }
    StoreGatherP p{t->actions, t->robot_obs, t->lang, reinterpret_cast<const long long*>(window_start), window_len, lang_row, actions_out, robot_obs_out, lang_out,
                   (long long)t->store_frames, t->lang_rows, B, S, t->absolute != 0};
    const int total = B * S * 22 + (lang_out ? B * 384 : 0);
    hipLaunchKernelGGL(store_gather_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->e->st, p);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_store_gather: launch failed"); return 1; }
    return 0;
}
int64_t hulc_store_stage(hulc_ctx* ctx, const hulc_stage_copy* copies, int32_t n) {
    if (!ctx) { hulc_set_error("hulc_store_stage: null context"); return -1; }
    return ctx->stager.stage(ctx->e->st, copies, n);
}
int hulc_store_stage_join(hulc_ctx* ctx, int64_t ticket) {
    if (!ctx) { hulc_set_error("hulc_store_stage_join: null context"); return 1; }
    return ctx->stager.join(ctx->e->st, ticket);
}
int hulc_store_stage_stats(hulc_ctx* ctx, int64_t* calls, int64_t* copies, int64_t* bytes) {
    if (!ctx) { hulc_set_error("hulc_store_stage_stats: null context"); return 1; }
    if (calls) *calls = ctx->stager.n_calls;
    if (copies) *copies = ctx->stager.n_copies;
    if (bytes) *bytes = ctx->stager.n_bytes;
    return 0;
}
int hulc_clip_gt_encode(hulc_ctx* ctx, const float* lang_emb, int32_t m, int32_t slot) {
    if (!ctx) { hulc_set_error("hulc_clip_gt_encode: null context"); return 1; }
    return ctx->e->clip_gt_encode(lang_emb, m, slot);
}
int hulc_clip_gt_scores(hulc_ctx* ctx, int32_t slot, float* scores_host, int64_t cap_floats, int32_t* n_out, int32_t* m_out) {
    if (!ctx) { hulc_set_error("hulc_clip_gt_scores: null context"); return 1; }
    return ctx->e->clip_gt_scores(slot, scores_host, cap_floats, n_out, m_out);
}
int hulc_aux_heads_enable(hulc_ctx* ctx, int32_t bc_z, int32_t mia) {
    if (!ctx) { hulc_set_error("hulc_aux_heads_enable: null context"); return 1; }
    return ctx->e->aux_heads_enable(bc_z, mia);
}
int hulc_decoder_select(hulc_ctx* ctx, int32_t decoder, int32_t criterion) {
    if (!ctx) { hulc_set_error("hulc_decoder_select: null context"); return 1; }
    return ctx->e->decoder_select(decoder, criterion);
}
int hulc_decoder_body_select(hulc_ctx* ctx, int32_t body) {
    if (!ctx) { hulc_set_error("hulc_decoder_body_select: null context"); return 1; }
    return ctx->e->decoder_body_select(body);
}
int hulc_aux_weights_set(hulc_ctx* ctx, float bc_z_weight, float mia_weight) {
    if (!ctx) { hulc_set_error("hulc_aux_weights_set: null context"); return 1; }
    return ctx->e->aux_weights_set(bc_z_weight, mia_weight);
}
int hulc_aux_losses_get(hulc_ctx* ctx, float* out_host) {
    if (!ctx) { hulc_set_error("hulc_aux_losses_get: null context"); return 1; }
    return ctx->e->aux_losses_get(out_host);
}
int hulc_rollout_reset(hulc_ctx* ctx) { return ctx->e->rollout_reset(); }
int hulc_rollout_plan(hulc_ctx* ctx, const hulc_rollout_obs* obs, const float* goal_rgb_static, const float* goal_rgb_gripper, const float* goal_lang,
                      const int32_t* plan_idx_inject, int32_t* plan_idx_out) {
    if (!obs || !obs->rgb_static || !obs->rgb_gripper) { hulc_set_error("hulc_rollout_plan: null observation"); return 1; }
    return ctx->e->rollout_plan(obs, goal_rgb_static, goal_rgb_gripper, goal_lang, plan_idx_inject, plan_idx_out);
}
int hulc_rollout_get_goal(hulc_ctx* ctx, float* latent_goal_out) {
    if (!latent_goal_out) { hulc_set_error("hulc_rollout_get_goal: null output"); return 1; }
    return ctx->e->rollout_get_goal(latent_goal_out);
}
int hulc_rollout_set_state(hulc_ctx* ctx, const void* plan, const float* latent_goal) {
    if (!latent_goal) { hulc_set_error("hulc_rollout_set_state: null latent goal"); return 1; }
    return ctx->e->rollout_set_state(plan, latent_goal);
}
int hulc_rollout_act(hulc_ctx* ctx, const hulc_rollout_obs* obs, const float* u_mix, const float* u_act, float* action_out_host) {
    if (!obs || !obs->rgb_static || !obs->rgb_gripper || !obs->robot_obs_raw || !action_out_host) { hulc_set_error("hulc_rollout_act: null argument"); return 1; }
    return ctx->e->rollout_act(obs, u_mix, u_act, action_out_host);
}
int hulc_rollout_envs_init(hulc_ctx* ctx, int32_t max_envs) {
    if (!ctx) { hulc_set_error("hulc_rollout_envs_init: null context"); return 1; }
    return ctx->e->rollout_envs_init(max_envs);
}
int hulc_rollout_envs_reset(hulc_ctx* ctx, int32_t n, const int32_t* slots, int32_t clear_hidden) {
    if (!ctx) { hulc_set_error("hulc_rollout_envs_reset: null context"); return 1; }
    return ctx->e->rollout_envs_reset(n, slots, clear_hidden);
}
int hulc_rollout_envs_plan(hulc_ctx* ctx, const hulc_rollout_envs_obs* obs, const float* goal_rgb_static, const float* goal_rgb_gripper, const float* goal_lang,
                           const void* plan_inject, void* plan_out, float* latent_goal_out) {
    if (!ctx || !obs || !obs->rgb_static || !obs->rgb_gripper) { hulc_set_error("hulc_rollout_envs_plan: null observation"); return 1; }
    return ctx->e->rollout_envs_plan(obs, goal_rgb_static, goal_rgb_gripper, goal_lang, plan_inject, plan_out, latent_goal_out);
}
int hulc_rollout_envs_act(hulc_ctx* ctx, const hulc_rollout_envs_obs* obs, const float* u_mix, const float* u_act, float* actions_out_host) {
    if (!ctx || !obs || !obs->rgb_static || !obs->rgb_gripper || !obs->robot_obs_raw || !actions_out_host) { hulc_set_error("hulc_rollout_envs_act: null argument"); return 1; }
    return ctx->e->rollout_envs_act(obs, u_mix, u_act, actions_out_host);
}
int hulc_rollout_envs_get_state(hulc_ctx* ctx, int32_t n, const int32_t* slots, void* plan_out, float* latent_goal_out) {
    if (!ctx) { hulc_set_error("hulc_rollout_envs_get_state: null context"); return 1; }
    return ctx->e->rollout_envs_get_state(n, slots, plan_out, latent_goal_out);
}
int hulc_rollout_envs_set_state(hulc_ctx* ctx, int32_t n, const int32_t* slots, const void* plan, const float* latent_goal) {
    if (!ctx || !latent_goal) { hulc_set_error("hulc_rollout_envs_set_state: null latent goal"); return 1; }
    return ctx->e->rollout_envs_set_state(n, slots, plan, latent_goal);
}
int hulc_sbert_create(const hulc_sbert_config* cfg, hulc_sbert** out) {
    if (!cfg || !out) { hulc_set_error("hulc_sbert_create: null argument"); return 1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { hulc_set_error("hulc_sbert_create: no HIP device visible"); return 1; }
    if (cfg->hidden % 64 != 0 || cfg->hidden > 1024 || cfg->hidden % cfg->heads != 0 || cfg->hidden / cfg->heads > 64 || cfg->max_tokens > 128 || cfg->layers < 1) {
        hulc_set_error("hulc_sbert_create: unsupported shape (hidden %% 64 == 0, <= 1024; head dim <= 64; <= 128 tokens)");
        return 1;
    }
    hulc_sbert* c = new hulc_sbert();
    c->cfg = *cfg;
    if (!c->init()) { delete c; hulc_set_error("hulc_sbert_create: workspace allocation failed"); return 1; }
    *out = c;
    return 0;
}
int hulc_sbert_destroy(hulc_sbert* ctx) { delete ctx; return 0; }
int hulc_sbert_set_stream(hulc_sbert* ctx, void* s) { ctx->st = (hipStream_t)s; return 0; }
int hulc_sbert_bind(hulc_sbert* ctx, const float* flat, int64_t numel, int32_t n, const char* const* names, const int64_t* offs, const int64_t* numels) {
    if (!ctx || !flat || !names || !offs || !numels) { hulc_set_error("hulc_sbert_bind: null argument"); return 1; }
    ctx->w.clear();
    for (int i = 0; i < n; ++i) {
        if (offs[i] < 0 || offs[i] + numels[i] > numel) { hulc_set_error("hulc_sbert_bind: tensor %s out of range", names[i]); return 1; }
        ctx->w[names[i]] = flat + offs[i];
    }
    const long long H = ctx->cfg.hidden, I = ctx->cfg.intermediate;
    auto need = [&](const std::string& nm, long long cnt) {
        for (int i = 0; i < n; ++i)
            if (nm == names[i]) return numels[i] == cnt;
        return false;
    };
    bool ok = need("embeddings.word_embeddings.weight", (long long)ctx->cfg.vocab * H) && need("embeddings.position_embeddings.weight", (long long)ctx->cfg.max_position * H) &&
              need("embeddings.LayerNorm.weight", H) && need("embeddings.LayerNorm.bias", H);
    for (int l = 0; l < ctx->cfg.layers && ok; ++l) {
        const std::string p = "encoder.layer." + std::to_string(l) + ".";
        ok = need(p + "attention.self.query.weight", H * H) && need(p + "attention.self.key.weight", H * H) && need(p + "attention.self.value.weight", H * H) &&
             need(p + "attention.self.query.bias", H) && need(p + "attention.self.key.bias", H) && need(p + "attention.self.value.bias", H) &&
             need(p + "attention.output.dense.weight", H * H) && need(p + "attention.output.dense.bias", H) && need(p + "attention.output.LayerNorm.weight", H) &&
             need(p + "attention.output.LayerNorm.bias", H) && need(p + "intermediate.dense.weight", I * H) && need(p + "intermediate.dense.bias", I) &&
             need(p + "output.dense.weight", H * I) && need(p + "output.dense.bias", H) && need(p + "output.LayerNorm.weight", H) && need(p + "output.LayerNorm.bias", H);
    }
    if (!ok || !ctx->get("embeddings.token_type_embeddings.weight")) { hulc_set_error("hulc_sbert_bind: a BertModel tensor is missing or has the wrong size"); return 1; }
    ctx->bound = true;
    return 0;
}
int hulc_sbert_encode(hulc_sbert* ctx, const int32_t* ids, const int32_t* mask, int32_t B, int32_t L, float* out) {
    if (!ctx || !ids || !mask || !out) { hulc_set_error("hulc_sbert_encode: null argument"); return 1; }
    return ctx->encode(ids, mask, B, L, out);
}
int hulc_adam_step(hulc_ctx* ctx, float lr, float b1, float b2, float eps, int64_t step, float gs) { return ctx->e->adam(lr, b1, b2, eps, step, gs); }
int hulc_optimizer_step(hulc_ctx* ctx, const hulc_optim* opt) {
    if (!ctx || !opt) { hulc_set_error("hulc_optimizer_step: null argument"); return 1; }
    return ctx->e->optim(*opt);
}
int hulc_comm_unique_id(void* out, int64_t cap) {
    if (!out || cap < 128) { hulc_set_error("hulc_comm_unique_id: need a 128-byte buffer"); return 1; }
    if (!GradComm::load_api()) return 1;
    GradComm::UniqueId id;
    const int rc = GradComm::api().get_id(&id);
    if (rc != 0) { hulc_set_error("ncclGetUniqueId failed: %s", GradComm::err(rc)); return 1; }
    memcpy(out, &id, 128);
    return 0;
}
int hulc_comm_prepare(hulc_ctx* ctx) {
    if (!ctx) { hulc_set_error("hulc_comm_prepare: null context"); return 1; }
    return ctx->e->comm_prepare();
}
int hulc_comm_init(hulc_ctx* ctx, const void* unique_id, int32_t rank, int32_t world) {
    if (!ctx || !unique_id || world < 1 || rank < 0 || rank >= world) { hulc_set_error("hulc_comm_init: bad argument"); return 1; }
    return ctx->e->comm_init(unique_id, rank, world);
}
int hulc_comm_destroy(hulc_ctx* ctx) { return ctx ? ctx->e->comm_destroy() : 0; }
int hulc_comm_buckets(hulc_ctx* ctx, int64_t* lo, int64_t* hi, int32_t cap) {
    if (!ctx || !lo || !hi) { hulc_set_error("hulc_comm_buckets: null argument"); return -1; }
    return ctx->e->comm_buckets(lo, hi, cap);
}
int hulc_comm_stats(hulc_ctx* ctx, int64_t* n_collectives, double* bytes) {
    if (!ctx || !ctx->e->comm) { hulc_set_error("hulc_comm_stats: no communicator"); return 1; }
    if (n_collectives) *n_collectives = ctx->e->comm->n_collectives;
    if (bytes) *bytes = ctx->e->comm->bytes_reduced;
    return 0;
}
int hulc_comm_size(hulc_ctx* ctx, int32_t* rank, int32_t* world) {
    if (!ctx || !ctx->e->comm) { hulc_set_error("hulc_comm_size: no communicator"); return 1; }
    int r = -1, w = -1;
    if (ctx->e->comm->size(&r, &w)) return 1;
    if (rank) *rank = r;
    if (world) *world = w;
    return 0;
}
int hulc_comm_timeline(hulc_ctx* ctx, double* out, int32_t cap_buckets, double* backward_us) {
    if (!ctx || !ctx->e->comm || !out) { hulc_set_error("hulc_comm_timeline: no communicator / null buffer"); return -1; }
    return ctx->e->comm->timeline(out, cap_buckets, backward_us, ctx->e->st);
}
int hulc_allreduce_grads(hulc_ctx* ctx, int32_t bucket_dtype) {
    if (!ctx) { hulc_set_error("hulc_allreduce_grads: null context"); return 1; }
    return ctx->e->allreduce_grads(bucket_dtype);
}
int hulc_backward_allreduce(hulc_ctx* ctx, int32_t bucket_dtype) {
    if (!ctx) { hulc_set_error("hulc_backward_allreduce: null context"); return 1; }
    return ctx->e->backward_allreduce(bucket_dtype);
}
int hulc_scaler_enable(hulc_ctx* ctx, float init_scale, float growth_factor, float backoff_factor, int32_t growth_interval) {
    if (!ctx) { hulc_set_error("hulc_scaler_enable: null context"); return 1; }
    return ctx->e->scaler_enable(init_scale, growth_factor, backoff_factor, growth_interval);
}
int hulc_scaler_get(hulc_ctx* ctx, float* scale, int32_t* growth_tracker, int64_t* skipped_steps, int32_t* last_found_inf, int64_t* taken_steps) {
    if (!ctx) { hulc_set_error("hulc_scaler_get: null context"); return 1; }
    return ctx->e->scaler_get(scale, growth_tracker, skipped_steps, last_found_inf, taken_steps);
}
int hulc_scaler_set(hulc_ctx* ctx, float scale, int32_t growth_tracker, int64_t taken_steps) {
    if (!ctx) { hulc_set_error("hulc_scaler_set: null context"); return 1; }
    return ctx->e->scaler_set(scale, growth_tracker, taken_steps);
}
int hulc_grad_clip_set(hulc_ctx* ctx, int32_t algo, float limit, int32_t track) {
    if (!ctx) { hulc_set_error("hulc_grad_clip_set: null context"); return 1; }
    return ctx->e->grad_clip_set(algo, limit, track);
}
int hulc_grad_norm_get(hulc_ctx* ctx, float* total, float* coef, float* per_tensor_host, int64_t cap) {
    if (!ctx) { hulc_set_error("hulc_grad_norm_get: null context"); return 1; }
    return ctx->e->grad_norm_get(total, coef, per_tensor_host, cap);
}
int hulc_trainable_set(hulc_ctx* ctx, int32_t n_tensors, const uint8_t* trainable) {
    if (!trainable) { hulc_set_error("hulc_trainable_set: null mask"); return 1; }      // the arguments first: each refusal is reachable without a device
    if (!ctx) { hulc_set_error("hulc_trainable_set: null context"); return 1; }
    return ctx->e->trainable_set(n_tensors, trainable);
}
int hulc_trainable_get(hulc_ctx* ctx, int64_t cap, uint8_t* trainable_out, int64_t* frozen_steps_out) {
    if (!ctx) { hulc_set_error("hulc_trainable_get: null context"); return 1; }
    return ctx->e->trainable_get(cap, trainable_out, frozen_steps_out);
}
int hulc_trainable_steps_set(hulc_ctx* ctx, int32_t n_tensors, const int64_t* frozen_steps, int64_t steps_taken) {
    if (!frozen_steps) { hulc_set_error("hulc_trainable_steps_set: null counts"); return 1; }
    if (!ctx) { hulc_set_error("hulc_trainable_steps_set: null context"); return 1; }
    return ctx->e->trainable_steps_set(n_tensors, frozen_steps, steps_taken);
}
int hulc_ema_enable(hulc_ctx* ctx, float* ema, float decay, int64_t start_step, int32_t warmup) {
    // the arguments first: the refusal is reachable without a device
    if (ema && (!(decay > 0.f && decay < 1.f) || start_step < 0)) { hulc_set_error("hulc_ema_enable: need 0 < decay < 1 and start_step >= 0 (got %g, %lld)", (double)decay, (long long)start_step); return 1; }
    if (!ctx) { hulc_set_error("hulc_ema_enable: null context"); return 1; }
    return ctx->e->ema_enable(ema, decay, start_step, warmup);
}
int hulc_ema_state_get(hulc_ctx* ctx, int64_t* updates, float* last_decay) {
    if (!ctx) { hulc_set_error("hulc_ema_state_get: null context"); return 1; }
    return ctx->e->ema_state_get(updates, last_decay);
}
int hulc_ema_state_set(hulc_ctx* ctx, int64_t updates) {
    if (updates < 0) { hulc_set_error("hulc_ema_state_set: updates %lld is negative", (long long)updates); return 1; }
    if (!ctx) { hulc_set_error("hulc_ema_state_set: null context"); return 1; }
    return ctx->e->ema_state_set(updates);
}
int hulc_ema_swap(hulc_ctx* ctx) {
    if (!ctx) { hulc_set_error("hulc_ema_swap: null context"); return 1; }
    return ctx->e->ema_swap();
}
int hulc_ema_swapped(hulc_ctx* ctx, int32_t* out) {
    if (!ctx || !out) { hulc_set_error("hulc_ema_swapped: null argument"); return 1; }
    return ctx->e->ema_is_swapped(out);
}
int hulc_set_kl_beta(hulc_ctx* ctx, float b) { ctx->e->set_kl_beta(b); return 0; }
int hulc_set_dropout(hulc_ctx* ctx, float p) {
    if (!(p >= 0.f && p < 1.f)) { hulc_set_error("hulc_set_dropout: p must be in [0,1)"); return 1; }      // NaN is refused too
    ctx->e->set_dropout(p);
    return 0;
}
int hulc_set_option(hulc_ctx* ctx, const char* name, int64_t value) {
    if (!ctx) { hulc_set_error("hulc_set_option: null context"); return 1; }
    return ctx->e->set_option(name, (long long)value);
}
int hulc_get_option(hulc_ctx* ctx, const char* name, int64_t* value) {
    if (!ctx || !value) { hulc_set_error("hulc_get_option: null argument"); return 1; }
    if (name && !strcmp(name, "stage_tickets")) { *value = HULC_STAGE_TICKETS; return 0; }      // the event ring of hulc_store_stage, as compiled
    long long v = 0;
    const int rc = ctx->e->get_option(name, &v);
    *value = (int64_t)v;
    return rc;
}
int hulc_timers_enable(hulc_ctx* ctx, int32_t on, const char* only_class) { ctx->e->set_timing(on != 0, only_class); return 0; }
int hulc_timers_read(hulc_ctx* ctx, char* json_out, int64_t cap, int32_t reset) { return ctx->e->timers_read(json_out, cap, reset != 0); }
int hulc_get_tensor(hulc_ctx* ctx, const char* name, float* out, int64_t cap, int64_t* n) { return ctx->e->get_tensor(name, out, cap, n); }
int hulc_get_plan_idx(hulc_ctx* ctx, int32_t* out, int64_t cap) { return ctx->e->get_plan_idx(out, cap); }

int hulc_k_gemm_nt(int32_t dtype, const void* A, const void* B, float* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                   const float* bias, int32_t relu, void* stream) {
    if (dtype == HULC_DTYPE_F16) return hulc_f16::k_gemm_nt(0, A, B, C, M, N, K, lda, ldb, ldc, bias, relu, stream);
    return hulc_bf16::k_gemm_nt(dtype == HULC_DTYPE_F32, A, B, C, M, N, K, lda, ldb, ldc, bias, relu, stream);
}
// the 16-bit encoder head and the action loss (k_entries.h): dispatched on dtype like hulc_k_gemm_nt
#define HULC_K_16BIT(name, call)                                                                                          \
    if (dtype == HULC_DTYPE_F16) return hulc_f16::call;                                                                    \
    if (dtype == HULC_DTYPE_BF16) return hulc_bf16::call;                                                                  \
    hulc_set_error(name ": dtype %d is not a 16-bit type", (int)dtype);                                                    \
    return 1
int hulc_k_spatial_softmax64(int32_t dtype, const void* f, int32_t H, int32_t W, int32_t Nf, void* out, float* stats, const float* dout, void* df, void* stream) {
    HULC_K_16BIT("hulc_k_spatial_softmax64", k_spatial_softmax64(f, H, W, Nf, out, stats, dout, df, stream));
}
int hulc_k_enc_tail_fwd(int32_t dtype, int32_t Nf, int32_t ldemb, const hulc_enc_tail_job* a, const hulc_enc_tail_job* b, void* emb, const float* pos, int32_t S,
                        float drop_p, uint64_t seed, float* xf, void* xt, float* z0, float* z1, void* stream) {
    HULC_K_16BIT("hulc_k_enc_tail_fwd", k_enc_tail_fwd(Nf, ldemb, a, b, emb, pos, S, drop_p, (unsigned long long)seed, xf, xt, z0, z1, stream));
}
int hulc_k_enc_tail_bwd(int32_t dtype, int32_t Nf, int32_t ldemb, const hulc_enc_tail_bwd_job* a, const hulc_enc_tail_bwd_job* b, const float* demb, void* stream) {
    HULC_K_16BIT("hulc_k_enc_tail_bwd", k_enc_tail_bwd(Nf, ldemb, a, b, demb, stream));
}
// the fused transformer layer kernels (tr_fused.h): 16-bit units only
int hulc_k_tr_layer_fwd(int32_t dtype, const hulc_tr_layer_job* job, int32_t B, int32_t S, int32_t ln_in, float dp, void* stream) {
    HULC_K_16BIT("hulc_k_tr_layer_fwd", k_tr_layer_fwd(job, B, S, ln_in, dp, stream));
}
int hulc_k_tr_ffn_bwd(int32_t dtype, const hulc_tr_ffn_bwd_job* job, int32_t B, int32_t S, int32_t bcast, float bdiv, float dp, void* stream) {
    HULC_K_16BIT("hulc_k_tr_ffn_bwd", k_tr_ffn_bwd(job, B, S, bcast, bdiv, dp, stream));
}
int hulc_k_tr_attn_bwd(int32_t dtype, const hulc_tr_attn_bwd_job* job, int32_t B, int32_t S, int32_t nparts, int64_t part_stride, float dp, void* stream) {
    HULC_K_16BIT("hulc_k_tr_attn_bwd", k_tr_attn_bwd(job, B, S, nparts, (long long)part_stride, dp, stream));
}
int hulc_k_gemm_dual(int32_t dtype, const hulc_gemm_epi_job* jobs, int32_t* ran, void* stream) {
    HULC_K_16BIT("hulc_k_gemm_dual", k_gemm_dual(jobs, ran, stream));
}
int hulc_k_lin_bwd_stream(int32_t dtype, const void* dY, const void* X, int64_t ldx, int32_t M, int32_t N, int32_t K, int32_t nsplit, int32_t store, float* dW, int64_t lddw,
                          float* db, float* slabs, void* stream) {
    HULC_K_16BIT("hulc_k_lin_bwd_stream", k_lin_bwd_stream(dY, X, (long long)ldx, M, N, K, nsplit, store, dW, (long long)lddw, db, slabs, stream));
}
#undef HULC_K_16BIT
// the GEMM core with its epilogue (k_entries.h): fp32 and bf16 instances in this unit, fp16 in the other
int hulc_k_gemm_epi(int32_t dtype, const hulc_gemm_epi_job* job, int32_t kernel, int32_t* ran, void* stream) {
    if (dtype == HULC_DTYPE_F16) return hulc_f16::k_gemm_epi(1, job, kernel, ran, stream);
    if (dtype != HULC_DTYPE_F32 && dtype != HULC_DTYPE_BF16) { hulc_set_error("hulc_k_gemm_epi: unknown dtype %d", (int)dtype); return 1; }
    return hulc_bf16::k_gemm_epi(dtype == HULC_DTYPE_BF16 ? 1 : 0, job, kernel, ran, stream);
}
int hulc_k_gemm_pick(int32_t dtype, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int32_t* pick, int32_t* bk) {
    if (dtype != HULC_DTYPE_F32 && dtype != HULC_DTYPE_BF16 && dtype != HULC_DTYPE_F16) { hulc_set_error("hulc_k_gemm_pick: unknown dtype %d", (int)dtype); return 1; }
    return hulc_bf16::k_gemm_pick(dtype != HULC_DTYPE_F32, M, N, K, (long long)lda, (long long)ldb, pick, bk);      // the routing does not depend on which 16-bit type
}
int hulc_k_gemm_wgrad_nsplit(int32_t dtype, int32_t M, int32_t N, int32_t K, int32_t* nsplit, int32_t* big) {
    if (dtype != HULC_DTYPE_F32 && dtype != HULC_DTYPE_BF16 && dtype != HULC_DTYPE_F16) { hulc_set_error("hulc_k_gemm_wgrad_nsplit: unknown dtype %d", (int)dtype); return 1; }
    return hulc_bf16::k_gemm_wgrad_nsplit(dtype != HULC_DTYPE_F32, M, N, K, nsplit, big);
}
int hulc_k_logistic_loss(int32_t dtype, int32_t wide, const float* heads, int32_t ldh, const float* actions, const float* robot_obs, int32_t B, int32_t S,
                         int32_t n_mix, int32_t n_dim, int32_t num_classes, float log_scale_min, float gripper_alpha, int32_t gripper_control,
                         int32_t discrete_gripper, float grad_scale, const float* lscale, float* row_loss, float* a_tcp_out, void* dheads, void* stream) {
    if (dtype == HULC_DTYPE_F16)
        return hulc_f16::k_logistic_loss(1, wide, heads, ldh, actions, robot_obs, B, S, n_mix, n_dim, num_classes, log_scale_min, gripper_alpha, gripper_control,
                                         discrete_gripper, grad_scale, lscale, row_loss, a_tcp_out, dheads, stream);
    if (dtype != HULC_DTYPE_F32 && dtype != HULC_DTYPE_BF16) { hulc_set_error("hulc_k_logistic_loss: unknown dtype %d", (int)dtype); return 1; }
    return hulc_bf16::k_logistic_loss(dtype == HULC_DTYPE_BF16, wide, heads, ldh, actions, robot_obs, B, S, n_mix, n_dim, num_classes, log_scale_min, gripper_alpha,
                                      gripper_control, discrete_gripper, grad_scale, lscale, row_loss, a_tcp_out, dheads, stream);
}
// the latent-plan kernels and the LayerNorm family (k_entries.h): fp32 and bf16 instances in this unit, fp16 in the other; the first argument of the entry is
// "16-bit type of the unit" (1) or float (0)
#define HULC_K_ANY(name, fn, ...)                                                                                                     \
    if (dtype == HULC_DTYPE_F16) return hulc_f16::fn(1, __VA_ARGS__);                                                                  \
    if (dtype != HULC_DTYPE_F32 && dtype != HULC_DTYPE_BF16) { hulc_set_error(name ": unknown dtype %d", (int)dtype); return 1; }      \
    return hulc_bf16::fn(dtype == HULC_DTYPE_BF16 ? 1 : 0, __VA_ARGS__)
int hulc_k_plan_kl_sample(const float* pr_logits, const float* pp_logits, int32_t B, int32_t NCAT, int32_t NCLS, const int32_t* idx_in, int32_t* idx_out, float* probs,
                          float* kl_cat, float* dpp, float* dpr, float w_pp, float w_pr, uint64_t seed, const float* lscale, void* stream) {
    return hulc_bf16::k_plan_kl_sample(pr_logits, pp_logits, B, NCAT, NCLS, idx_in, idx_out, probs, kl_cat, dpp, dpr, w_pp, w_pr, (unsigned long long)seed, lscale, stream);
}
int hulc_k_st_softmax_bwd(int32_t dtype, const float* probs, const float* dplan, const float* dpr_kl, const float* dpp_kl, int32_t rows, int32_t NCLS, float* out, void* out_t,
                          void* dpp_t, void* stream) {
    HULC_K_ANY("hulc_k_st_softmax_bwd", k_st_softmax_bwd, probs, dplan, dpr_kl, dpp_kl, rows, NCLS, out, out_t, dpp_t, stream);
}
int hulc_k_plan_gather(int32_t dtype, const void* w_t, const int32_t* idx, int32_t B, int32_t NCAT, int32_t NCLS, int32_t H, const float* b1, const float* b2, float* out,
                       const void* emb, void* embg, int32_t S, int32_t W, const void* goal, int32_t G, int32_t grow0, void* cb, void* stream) {
    HULC_K_ANY("hulc_k_plan_gather", k_plan_gather, w_t, idx, B, NCAT, NCLS, H, b1, b2, out, emb, embg, S, W, goal, G, grow0, cb, stream);
}
int hulc_k_plan_scatter_grad(int32_t dtype, int32_t form, const void* dC, const int32_t* idx, int32_t B, int32_t NCAT, int32_t NCLS, int32_t H, int32_t KIN, float* dw,
                             int32_t store, void* stream) {
    HULC_K_ANY("hulc_k_plan_scatter_grad", k_plan_scatter_grad, form, dC, idx, B, NCAT, NCLS, H, KIN, dw, store, stream);
}
int hulc_k_normal_kl_sample(int32_t dtype, const float* pr_state, const float* pp_state, int32_t B, int32_t n, const float* eps_in, float* eps_out, float* plan_f, void* plan_t,
                            float* kl_elem, float* dpp, float* dpr, float w_pp, float w_pr, uint64_t seed, const float* lscale, void* stream) {
    HULC_K_ANY("hulc_k_normal_kl_sample", k_normal_kl_sample, pr_state, pp_state, B, n, eps_in, eps_out, plan_f, plan_t, kl_elem, dpp, dpr, w_pp, w_pr, (unsigned long long)seed, lscale, stream);
}
int hulc_k_normal_rsample_bwd(int32_t dtype, const float* dplan, const float* eps, const float* pr_state, const float* dpr_kl, int32_t B, int32_t n, void* out, void* stream) {
    HULC_K_ANY("hulc_k_normal_rsample_bwd", k_normal_rsample_bwd, dplan, eps, pr_state, dpr_kl, B, n, out, stream);
}
// the deterministic decoder's head (det_head.h)
int hulc_k_det_head_loss(int32_t dtype, const void* H1, const void* W, const float* bias, const float* actions, const float* robot_obs, int32_t B, int32_t S,
                         int32_t criterion, int32_t frame, float grad_scale, const float* lscale, float* row_loss, float* pred, float* dpre, void* stream) {
    HULC_K_ANY("hulc_k_det_head_loss", k_det_head_loss, H1, W, bias, actions, robot_obs, B, S, criterion, frame, grad_scale, lscale, row_loss, pred, dpre, stream);
}
int hulc_k_det_head_bwd(int32_t dtype, const float* dpre, const void* W, const void* H1, int32_t B, int32_t S, void* dH1, void* dZ1, float* dW, float* db, void* stream) {
    HULC_K_ANY("hulc_k_det_head_bwd", k_det_head_bwd, dpre, W, H1, B, S, dH1, dZ1, dW, db, stream);
}
int hulc_k_det_head_act(int32_t dtype, const void* h1, const void* W, const float* bias, const float* robot_obs, int32_t n, float* out, void* stream) {
    HULC_K_ANY("hulc_k_det_head_act", k_det_head_act, h1, W, bias, robot_obs, n, out, stream);
}
int hulc_k_layernorm_fwd(int32_t dtype, const float* x, int64_t ldx, int32_t rows, int32_t n, const float* g, const float* b, void* out, int64_t ldo, float* out_f32, int64_t ldf,
                         float* stats, void* stream) {
    HULC_K_ANY("hulc_k_layernorm_fwd", k_layernorm_fwd, x, (long long)ldx, rows, n, g, b, out, (long long)ldo, out_f32, (long long)ldf, stats, stream);
}
int hulc_k_layernorm_bwd(int32_t dtype, const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* stats, const float* g, int32_t rows, int32_t n, float* dx_f32,
                         int64_t ldd, int32_t accumulate, void* dx_t, int64_t ldt, float* dg, float* db, float drop_p, uint64_t seed, int32_t bcast_rows, float bcast_div,
                         int32_t dy_parts, int64_t dy_part_stride, float* scratch, void* stream) {
    HULC_K_ANY("hulc_k_layernorm_bwd", k_layernorm_bwd, dy, (long long)lddy, x, (long long)ldx, stats, g, rows, n, dx_f32, (long long)ldd, accumulate, dx_t, (long long)ldt, dg, db,
               drop_p, (unsigned long long)seed, bcast_rows, bcast_div, dy_parts, (long long)dy_part_stride, scratch, stream);
}
int hulc_k_layernorm_mean(int32_t dtype, const float* x, int32_t B, int32_t S, int32_t n, const float* g, const float* b, float* stats, void* out, float* yout, void* stream) {
    HULC_K_ANY("hulc_k_layernorm_mean", k_layernorm_mean, x, B, S, n, g, b, stats, out, yout, stream);
}
#undef HULC_K_ANY
int hulc_k_cast(int32_t dtype, const float* src, void* dst, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HULC_DTYPE_F32) hipLaunchKernelGGL((cast_kernel<float, float>), dim3(1024), dim3(256), 0, st, src, (float*)dst, (long long)n);
    else hipLaunchKernelGGL((cast_kernel<float, h16_t>), dim3(1024), dim3(256), 0, st, src, (h16_t*)dst, (long long)n);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_cast: launch failed"); return 1; }
    return 0;
}
// the averaged weights' update pass alone, through the optimizer step's launch (kernels.h launch_ema_update): chunks == 0 is the flat form over ema[0, n)
int hulc_k_ema_update(float* ema, const float* p, int64_t n, float w, const int64_t* chunk_start, const int32_t* chunk_n, int32_t chunks, void* stream) {
    if (!ema || !p || n < 1 || chunks < 0 || (chunks && (!chunk_start || !chunk_n)) || ((uintptr_t)ema | (uintptr_t)p) % 16) {
        hulc_set_error("hulc_k_ema_update: null or misaligned argument, or n=%lld, chunks=%d out of range", (long long)n, (int)chunks); return 1; }
    launch_ema_update((hipStream_t)stream, ema, p, (long long)n, nullptr, w, reinterpret_cast<const long long*>(chunk_start), chunk_n, chunks, nullptr, nullptr, 0);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_ema_update: launch failed"); return 1; }
    return 0;
}
// the row kernels of the ragged encoder pass (window_rows.h), through the engine's launchers.  lens / off are device arrays the caller built (ragged_plan)
int hulc_k_window_compact(const int64_t* window_start, const int32_t* lens, const int32_t* off, int32_t off_base, int32_t B, int32_t S, int64_t store_frames,
                          const int32_t* shift_static, const int32_t* shift_gripper, int64_t* frame_out, int32_t* shift_static_out, int32_t* shift_gripper_out, void* stream) {
    if (!window_start || !lens || !off || !frame_out || B < 1 || S < 1 || store_frames < 1 || (shift_static && !shift_static_out) || (shift_gripper && !shift_gripper_out)) {
        hulc_set_error("hulc_k_window_compact: null argument or B=%d, S=%d, store_frames=%lld out of range", (int)B, (int)S, (long long)store_frames); return 1; }
    launch_window_compact((hipStream_t)stream, reinterpret_cast<const long long*>(window_start), lens, off, off_base, B, S, (long long)store_frames, shift_static, shift_gripper,
                          reinterpret_cast<long long*>(frame_out), shift_static_out, shift_gripper_out);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_window_compact: launch failed"); return 1; }
    return 0;
}
int hulc_k_rows_expand(int32_t elem_bytes, const void* src, const int32_t* lens, const int32_t* off, int32_t B, int32_t S, int32_t n, void* dst, void* stream) {
    if (!src || !lens || !off || !dst || B < 1 || S < 1 || n < 1 || (elem_bytes != 2 && elem_bytes != 4) || (n * elem_bytes) % 16 || ((uintptr_t)src | (uintptr_t)dst) % 16) {
        hulc_set_error("hulc_k_rows_expand: null or misaligned argument, or B=%d, S=%d, n=%d, elem_bytes=%d unsupported", (int)B, (int)S, (int)n, (int)elem_bytes); return 1; }
    if (elem_bytes == 4) launch_rows_expand<float>((hipStream_t)stream, (const float*)src, lens, off, B, S, n, (float*)dst);
    else launch_rows_expand<h16_t>((hipStream_t)stream, (const h16_t*)src, lens, off, B, S, n, (h16_t*)dst);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_rows_expand: launch failed"); return 1; }
    return 0;
}
int hulc_k_rows_reduce(const float* src, const int32_t* lens, const int32_t* off, int32_t B, int32_t S, int32_t n, float* dst, void* stream) {
    if (!src || !lens || !off || !dst || B < 1 || S < 1 || n < 4 || n % 4 || ((uintptr_t)src | (uintptr_t)dst) % 16) {
        hulc_set_error("hulc_k_rows_reduce: null or misaligned argument, or B=%d, S=%d, n=%d unsupported", (int)B, (int)S, (int)n); return 1; }
    launch_rows_reduce((hipStream_t)stream, src, lens, off, B, S, n, dst);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_rows_reduce: launch failed"); return 1; }
    return 0;
}

// the language auxiliary losses alone, routed on n as the engines route them (aux_rows.h): n <= 64 runs the single-workgroup kernels.  Synchronise.
static int k_clip_loss(bool wide, const float* img, const float* txt, int32_t n, const float* logit_scale, float w, float* loss_out, float* dimg, float* dtxt,
                       float* dlogit_scale, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || !img || !txt || !logit_scale || !loss_out || !dimg || !dtxt || !dlogit_scale) { hulc_set_error("hulc_k_clip_loss: n=%d or a null argument", (int)n); return 1; }
    float* ws = nullptr;
    if (n > AUX_ROWS_SINGLE && hipMalloc((void**)&ws, sizeof(float) * (size_t)clip_rows_ws_floats(n)) != hipSuccess) { hulc_set_error("hulc_k_clip_loss: hipMalloc failed"); return 1; }
    const bool ok = launch_clip_loss(st, wide, img, txt, n, logit_scale, w, loss_out, dimg, dtxt, dlogit_scale, nullptr, ws);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    if (ws) hipFree(ws);
    if (!ok || e1 != hipSuccess || e2 != hipSuccess) { hulc_set_error("hulc_k_clip_loss: %s", !ok ? "not launched" : hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return 1; }
    return 0;
}
int hulc_k_clip_loss(const float* img, const float* txt, int32_t n, const float* logit_scale, float w, float* loss_out, float* dimg, float* dtxt, float* dlogit_scale,
                     void* stream) { return k_clip_loss(true, img, txt, n, logit_scale, w, loss_out, dimg, dtxt, dlogit_scale, stream); }
int hulc_k_clip_loss_fp32(const float* img, const float* txt, int32_t n, const float* logit_scale, float w, float* loss_out, float* dimg, float* dtxt,
                          float* dlogit_scale, void* stream) { return k_clip_loss(false, img, txt, n, logit_scale, w, loss_out, dimg, dtxt, dlogit_scale, stream); }
int hulc_k_mia_head(const float* img, const float* txt, int32_t n, const float* W0, const float* b0, const float* W1, const float* b1, float w, float* loss_out,
                    float* dimg, float* dtxt, int32_t accum, float* dW0, float* db0, float* dW1, float* db1, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || !img || !txt || !W0 || !b0 || !W1 || !b1 || !loss_out) { hulc_set_error("hulc_k_mia_head: n=%d or a null argument", (int)n); return 1; }
    if (dW0 && (!dimg || !dtxt || !db0 || !dW1 || !db1)) { hulc_set_error("hulc_k_mia_head: the backward needs every gradient pointer"); return 1; }
    float* ws = nullptr;
    if (n > AUX_ROWS_SINGLE && hipMalloc((void**)&ws, sizeof(float) * (size_t)mia_rows_ws_floats(n)) != hipSuccess) { hulc_set_error("hulc_k_mia_head: hipMalloc failed"); return 1; }
    const bool ok = launch_mia_head(st, img, txt, n, W0, b0, W1, b1, w, loss_out, dimg, dtxt, accum, dW0, db0, dW1, db1, nullptr, ws);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    if (ws) hipFree(ws);
    if (!ok || e1 != hipSuccess || e2 != hipSuccess) { hulc_set_error("hulc_k_mia_head: %s", !ok ? "not launched" : hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return 1; }
    return 0;
}
int hulc_k_cosine_dist(const float* pred, const float* tgt, int32_t n, int32_t D, float w, float* loss_out, float* dpred, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || D < 1 || !pred || !tgt || !loss_out) { hulc_set_error("hulc_k_cosine_dist: n=%d D=%d or a null argument", (int)n, (int)D); return 1; }
    hipLaunchKernelGGL(cosine_dist_loss_kernel, dim3(1), dim3(1024), 0, st, pred, tgt, n, D, w, loss_out, dpred, (const float*)nullptr);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    if (e1 != hipSuccess || e2 != hipSuccess) { hulc_set_error("hulc_k_cosine_dist: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return 1; }
    return 0;
}

int hulc_k_attention(int32_t variant, const float* qkv, float* P, float* ao, const float* dao, float* dqkv, int32_t B, int32_t S, float drop_p,
                     uint64_t seed, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int D = 128, NH = 8;
    if (S < 1 || S > 64 || (variant == 1 && S > 32)) { hulc_set_error("hulc_k_attention: S=%d not covered by variant %d", S, variant); return 1; }
    // 1: two lanes per query row (the 16-bit engines' S <= 32 form); 2: four waves per (b, head) (their S > 32 form, here at any S <= 64); else: the fp32 engine's serial kernels
    const bool wide = variant == 1 || variant == 2, s64 = variant == 2 || (!wide && attention_s64(S));
    if (wide && !dao) launch_attention_fwd<float, true>(st, s64, qkv, B, S, D, NH, P, ao, drop_p, (unsigned long long)seed);
    else if (wide) launch_attention_bwd<float, true>(st, s64, qkv, P, dao, B, S, D, NH, dqkv, drop_p, (unsigned long long)seed);
    else if (!dao) launch_attention_fwd<float, false>(st, s64, qkv, B, S, D, NH, P, ao, drop_p, (unsigned long long)seed);
    else launch_attention_bwd<float, false>(st, s64, qkv, P, dao, B, S, D, NH, dqkv, drop_p, (unsigned long long)seed);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_attention: launch failed"); return 1; }
    return 0;
}

// The encoder's convolution family (k_entries.h: k_conv_wgrad, k_conv1_wgrad_u8, k_conv_tile, k_conv_pair, k_conv_plan).  The entries without a dtype are the bf16
// wrappers; the _t entries take HULC_DTYPE_BF16 or HULC_DTYPE_F16 and refuse anything else before anything is allocated or launched
#define HULC_K_CONV_T(name, call)                                                                                          \
    if (dtype == HULC_DTYPE_F16) return hulc_f16::call;                                                                    \
    if (dtype == HULC_DTYPE_BF16) return hulc_bf16::call;                                                                  \
    hulc_set_error(name ": dtype %d is not a 16-bit type (HULC_DTYPE_BF16 or HULC_DTYPE_F16)", (int)dtype);                \
    return 1
// conv wgrad unit-test entry (bf16 NHWC): out[CO][KH*KW*CI] (packed (kh,kw,ci) order, fp32, overwritten)
int hulc_k_conv_wgrad(int32_t which, const void* X, const void* dY, float* out, int32_t Nf, int32_t IH, void* stream) {
    return hulc_bf16::k_conv_wgrad("hulc_k_conv_wgrad", 0, which, X, dY, out, nullptr, Nf, IH, nullptr, stream);
}
int hulc_k_conv_wgrad_t(int32_t dtype, int32_t which, const void* X, const void* dY, float* out, float* db_out, int32_t Nf, int32_t IH, int32_t* slabs, void* stream) {
    HULC_K_CONV_T("hulc_k_conv_wgrad_t", k_conv_wgrad("hulc_k_conv_wgrad_t", 1, which, X, dY, out, db_out, Nf, IH, slabs, stream));
}

// host arithmetic only (no device needed): the interior group range the uint8 conv1 kernels convert without clamps (conv1_stage.h::conv1_interior_groups)
int hulc_k_conv1_interior_groups(int32_t IW, int32_t pad, int32_t cap, int32_t* first, int32_t* count) {
    int cl = 0, wi = 0;
    conv1_interior_groups(IW, pad, cap, cl, wi);
    *first = cl; *count = wi;
    return 0;
}

// conv1's weight gradient from uint8 (Nf,IH,IH,3) frames alone (tests): dW (32,192) [torch (o, c, kh, kw) order] and db (32)
int hulc_k_conv1_wgrad_u8(const void* X, const int32_t* shifts, int32_t pad, const void* dY, float* dw_out, float* db_out, int32_t Nf, int32_t IH, int32_t form, int32_t fold, void* stream) {
    return hulc_bf16::k_conv1_wgrad_u8("hulc_k_conv1_wgrad_u8", 0, X, shifts, pad, dY, dw_out, db_out, Nf, IH, form, fold, nullptr, stream);
}
int hulc_k_conv1_wgrad_u8_t(int32_t dtype, const void* X, const int32_t* shifts, int32_t pad, const void* dY, float* dw_out, float* db_out, int32_t Nf, int32_t IH, int32_t form,
                            int32_t fold, int32_t* slabs, void* stream) {
    HULC_K_CONV_T("hulc_k_conv1_wgrad_u8_t", k_conv1_wgrad_u8("hulc_k_conv1_wgrad_u8_t", 1, X, shifts, pad, dY, dw_out, db_out, Nf, IH, form, fold, slabs, stream));
}

// raw-tile conv kernels alone (bf16 NHWC): mode 0 fwd 3x3/s1 64->64, 1 fwd 4x4/s2 32->64, 2 dgrad of (0), 3 dgrad of (1); the other modes: include/hulc_hip.h
int hulc_k_conv_tile(int32_t mode, const void* img, const void* w, const float* bias, const void* mask, void* out, int32_t Nf, int32_t IMH,
                     int32_t OUTH, int32_t relu, void* stream) {
    return hulc_bf16::k_conv_tile("hulc_k_conv_tile", 0, mode, img, w, bias, mask, out, nullptr, Nf, IMH, OUTH, relu, 0, stream);
}
int hulc_k_conv_tile_t(int32_t dtype, int32_t mode, const void* img, const void* w, const float* bias, const void* mask, void* out, uint32_t* bits1_out, int32_t Nf, int32_t IMH,
                       int32_t OUTH, int32_t relu, int32_t wgs, void* stream) {
    HULC_K_CONV_T("hulc_k_conv_tile_t", k_conv_tile("hulc_k_conv_tile_t", 1, mode, img, w, bias, mask, out, bits1_out, Nf, IMH, OUTH, relu, wgs, stream));
}
// host arithmetic only (no device needed): plan_conv_reg's band / stack geometry of a weights-in-registers form (the same for both 16-bit types)
int hulc_k_conv_plan(int32_t form, int32_t frames, int32_t in_side, int32_t out_side, int32_t wgs, int32_t* nbands, int32_t* rows_per_band, int32_t* frames_per_band, int32_t* items) {
    return hulc_bf16::k_conv_plan(form, frames, in_side, out_side, wgs, nbands, rows_per_band, frames_per_band, items);
}

// host arithmetic only (no device needed): the division of a launch's persistent workgroups between the two cameras' jobs (common.h::camera_split)
int hulc_k_camera_split(int32_t grid, double work_static, double work_gripper, int32_t* wg_static, int32_t* wg_gripper) {
    int a = 0, b = 0;
    camera_split(grid, work_static, work_gripper, a, b);
    *wg_static = a; *wg_gripper = b;
    return 0;
}

// One stage of both encoders as ONE launch, in the forms the engine runs (k_entries.h: k_conv_pair); b == NULL: job a alone through the same entry
int hulc_k_conv_pair(int32_t stage, const hulc_conv_job* a, const hulc_conv_job* b, int32_t wg_a, int32_t wg_b, void* stream) {
    return hulc_bf16::k_conv_pair("hulc_k_conv_pair", 0, stage, a, b, wg_a, wg_b, nullptr, stream);
}
int hulc_k_conv_pair_t(int32_t dtype, int32_t stage, const hulc_conv_job* a, const hulc_conv_job* b, int32_t wg_a, int32_t wg_b, int32_t* slabs, void* stream) {
    HULC_K_CONV_T("hulc_k_conv_pair_t", k_conv_pair("hulc_k_conv_pair_t", 1, stage, a, b, wg_a, wg_b, slabs, stream));
}
#undef HULC_K_CONV_T

// skinny GEMM alone (bf16): out[M][N] (bf16) = A[M][K] W[N][K]^T ; variant = NW*10 + MT (e.g. 82 = 8 waves, 32-row blocks)
int hulc_k_skinny(const void* A, const void* W, void* out, int32_t M, int32_t N, int32_t K, int32_t variant, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    EpiP ep; ep.out = out; ep.out_f32 = 0;
    const int NW = variant / 10, MT = variant % 10;
    dim3 grid(N / 16, MT > 0 ? (M + MT * 16 - 1) / (MT * 16) : 1);
    const h16_t* a = (const h16_t*)A; const h16_t* w = (const h16_t*)W;
#define SK(nw, mt) hipLaunchKernelGGL((skinny_gemm_kernel<nw, mt>), grid, dim3(nw * 64), 0, st, a, (long long)K, w, (long long)K, M, N, K, dense_out(N), ep)
    if (NW == 8 && MT == 2) SK(8, 2); else if (NW == 8 && MT == 4) SK(8, 4); else if (NW == 4 && MT == 2) SK(4, 2); else if (NW == 4 && MT == 4) SK(4, 4);
    else if (NW == 8 && MT == 1) SK(8, 1); else if (NW == 4 && MT == 1) SK(4, 1);
    else if (NW == 16 && MT == 2) SK(16, 2); else if (NW == 16 && MT == 4) SK(16, 4);
    else if (NW == 9 && MT == 2) hipLaunchKernelGGL((skinny_gemm_kernel<8, 2, 8>), grid, dim3(512), 0, st, a, (long long)K, w, (long long)K, M, N, K, dense_out(N), ep);
    else if (NW == 17 && MT == 2) hipLaunchKernelGGL((skinny_gemm_kernel<16, 2, 4>), grid, dim3(1024), 0, st, a, (long long)K, w, (long long)K, M, N, K, dense_out(N), ep);
    else if (NW == 20) { if (!launch_skinny_lds(st, a, (long long)K, w, (long long)K, M, N, K, MT, dense_out(N), ep)) { hulc_set_error("hulc_k_skinny: shape not covered by the LDS kernel"); return 1; } }
    else if (NW == 30) launch_skinny(st, a, (long long)K, w, (long long)K, M, N, K, dense_out(N), ep);       // the production router (incl. the K-chunked LDS kernel)
    else if (NW == 40) {      // two independent problems in one launch (the paired directions of a bidirectional recurrence): the second one lives at A + M*K, W + N*K, out + M*N
        EpiP ep2 = ep; ep2.out = (h16_t*)out + (long long)M * N;
        if (!launch_skinny_lds_dual(st, a, w, ep, a + (long long)M * K, w + (long long)N * K, ep2, (long long)K, (long long)K, M, N, K, dense_out(N))) {
            hulc_set_error("hulc_k_skinny: shape not covered by the dual launch"); return 1; }
    }
    else if (NW == 50 || NW == 51) {      // fragment-ordered weight copies (gemm.h: frag_pack_kernel).  500: W repacked into a scratch copy, then the K-chunked LDS kernel reads
        // it with ldw == 0 (K = n x 2048, M <= 64: the GRU's BPTT step);  510: the repacked W itself lands in `out` (N x K elements; K % 128 == 0, N % 16 == 0)
        if ((N % 16) != 0 || (K % 128) != 0) { hulc_set_error("hulc_k_skinny: fragment order needs N %% 16 == 0 and K %% 128 == 0"); return 1; }
        h16_t* wf = (h16_t*)out;
        if (NW == 50 && hipMalloc((void**)&wf, (size_t)N * K * sizeof(h16_t)) != hipSuccess) { hulc_set_error("hulc_k_skinny: scratch allocation failed"); return 1; }
        FragPackBatch fb{};
        fb.src[0] = w; fb.dst[0] = wf; fb.N[0] = N; fb.K[0] = K; fb.blk0[0] = 0; fb.blk0[1] = frag_pack_blocks(N, K); fb.n = 1;
        hipLaunchKernelGGL(frag_pack_kernel, dim3(fb.blk0[1]), dim3(256), 0, st, fb);
        if (NW == 50) {
            const bool ok = launch_skinny_lds_kchunk(st, a, (long long)K, wf, 0ll, M, N, K, dense_out(N), ep);
            hipStreamSynchronize(st);
            hipFree(wf);
            if (!ok) { hulc_set_error("hulc_k_skinny: shape not covered by the K-chunked kernel"); return 1; }
        }
    }
    else { hulc_set_error("hulc_k_skinny: unsupported variant"); return 1; }
#undef SK
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// one whole recurrence as a persistent launch (rnn_persist.h), bf16: X [S][B][2048] with X[q0] given; flags = RP_FLAG_WORDS zeroed uint32 words
// (reused across calls with increasing launch_index >= 1), err = one zeroed uint32
int hulc_k_rnn_persist(void* X, const void* W, const void* res, const void* mask, int32_t B, int32_t S, int32_t q0, int32_t dq, int32_t act, uint32_t* flags,
                       uint32_t* err, uint32_t launch_index, void* stream) {
    RnnPersistP p{};
    p.X = (h16_t*)X; p.W = (const h16_t*)W; p.res = (const h16_t*)res; p.mask = (const h16_t*)mask; p.B = B; p.S = S; p.q0 = q0; p.dq = dq; p.act = act;
    p.flags = flags; p.base = launch_index << 12; p.parity = (int)(launch_index & 1u); p.err = err; p.stamps = nullptr;
    if (!launch_rnn_persist((hipStream_t)stream, p)) { hulc_set_error("hulc_k_rnn_persist: shape not covered (S >= 2, B <= 128)"); return 1; }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
int32_t hulc_k_rnn_persist_flag_words(void) { return RP_FLAG_WORDS; }

// probe of ds_read_b64_tr_b16 semantics (tests/tools only): LDS image lds[i] = i (uint16), lane l reads at element index addr[l]
__global__ void trread_probe_kernel(const int* __restrict__ addr_in, unsigned short* __restrict__ out) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) unsigned short lds[8192];
    for (int i = threadIdx.x; i < 8192; i += 64) lds[i] = (unsigned short)i;
    __syncthreads();
    const int a = addr_in[threadIdx.x];
    s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + a));
#pragma unroll
    for (int j = 0; j < 4; ++j) out[threadIdx.x * 4 + j] = (unsigned short)v[j];
}
int hulc_k_trread_probe(const int32_t* addr, uint16_t* out, void* stream) {
    hipLaunchKernelGGL(trread_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)addr, (unsigned short*)out);
    if (hipGetLastError() != hipSuccess) { hulc_set_error("trread probe launch failed"); return 1; }
    return 0;
}

}  // extern "C"
