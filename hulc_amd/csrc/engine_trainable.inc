// hulc_amd/csrc/engine_trainable.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body: the per-tensor trainable
// mask (hulc_trainable_set / hulc_trainable_get / hulc_trainable_steps_set).  Not a standalone header.
//
// A context that never calls these entries keeps tm_active == false and runs exactly the launches it ran before they existed.  Once a mask is set, the optimizer
// step, the norm pass, the non-finite check and the post-step weight refresh run on TABLES that list the trainable tensors only (kernels.h adam_grouped_kernel,
// sgd_grouped_kernel; grad_sumsq_kernel over a chunk table without the frozen tensors): nothing of a frozen tensor — parameter, moments, gradient, 16-bit shadow,
// transposed / fragment-ordered / packed copies — is read or written by the step.  Every table is rebuilt here, never on the step path.
    bool tm_active = false;
    std::vector<std::string> tm_names;        // the bound tensors' names in bind order (gn_tens holds their ranges)
    std::vector<uint8_t> tm_mask;             // bind order, 1 = trainable
    // torch.optim keeps `step` per parameter.  Per tensor: trainable -> the optimizer steps it sat out so far (constant while it trains); frozen -> the steps it
    // has taken (constant while it is frozen).  The two are converted into each other with the count of steps taken at the moment of the switch.
    std::vector<int64_t> tm_cnt;
    int64_t tm_last_step = 0;                 // hulc_optim::step of the last optimizer step (engines without the loss scaler count through the caller)
    int tm_ntrain = 0, tm_ngroups = 0;
    int64_t tm_goff[OPT_GROUPS] = {};         // distinct sat-out counts among the trainable tensors
    std::vector<uint8_t> tm_gid;              // per tensor: its group
    bool tm_enc_frozen = false;               // every perceptual_encoder.* tensor is frozen: the backward stops behind part 0
    bool bwd_skip_enc = false;                // latched by the backward that runs part 0
    struct ChunkTable { long long* start = nullptr; int* n = nullptr; unsigned char* gid = nullptr; int chunks = 0; };
    ChunkTable tm_flat, tm_comp;              // every trainable tensor / the trainable tensors the tile pass does not cover
    TrTable tm_tiles, tm_tr_all, tm_tr_rest;  // trainable subsets of tr_adam, trdesc, tr_rest
    unsigned char* tm_tile_gid = nullptr;
    bool tm_tile_ok = false;                  // every tiled matrix is one whole bound tensor (else the masked step takes the chunk form + batched transposes)
    FragPackBatch tm_frag{}; int tm_frag_blocks = 0;
    std::vector<TrDesc> tr_fused_host, tr_rest_host;      // host copies of tr_adam / tr_rest (adam_tables_build)

    void chunk_table_free(ChunkTable& c) { if (c.start) hipFree(c.start); if (c.n) hipFree(c.n); if (c.gid) hipFree(c.gid); c = ChunkTable{}; }
    bool chunk_table_build(ChunkTable& c, const std::vector<int>& tensors) {
        chunk_table_free(c);
        std::vector<long long> cs; std::vector<int> cn; std::vector<unsigned char> cg;
        for (int t : tensors) {
            const Ref& r = gn_tens[t];
            // the tensor's last quad may reach into its own alignment padding (the flat kernels update padding too), never into the next tensor or past the buffer
            int64_t lim = numel;
            for (const Ref& o : gn_tens) if (o.off > r.off && o.off < lim) lim = o.off;
            const int64_t up = (r.n + 3) / 4 * 4, n4 = r.off + up <= lim ? up : (r.n & ~(int64_t)3);
            for (int64_t x = 0; x < n4; x += ADAM_CHUNK) { cs.push_back(r.off + x); cn.push_back((int)std::min<int64_t>(ADAM_CHUNK, n4 - x)); cg.push_back(tm_gid[t]); }
        }
        c.chunks = (int)cs.size();
        if (cs.empty()) return true;
        if (hipMalloc((void**)&c.start, sizeof(long long) * cs.size()) != hipSuccess || hipMalloc((void**)&c.n, sizeof(int) * cn.size()) != hipSuccess ||
            hipMalloc((void**)&c.gid, cg.size()) != hipSuccess) { chunk_table_free(c); return false; }
        hipMemcpy(c.start, cs.data(), sizeof(long long) * cs.size(), hipMemcpyHostToDevice);
        hipMemcpy(c.n, cn.data(), sizeof(int) * cn.size(), hipMemcpyHostToDevice);
        hipMemcpy(c.gid, cg.data(), cg.size(), hipMemcpyHostToDevice);
        return true;
    }
    void tm_free() {
        chunk_table_free(tm_flat); chunk_table_free(tm_comp);
        tr_table_free(tm_tiles); tr_table_free(tm_tr_all); tr_table_free(tm_tr_rest);
        if (tm_tile_gid) { hipFree(tm_tile_gid); tm_tile_gid = nullptr; }
        tm_frag = FragPackBatch{}; tm_frag_blocks = 0; tm_tile_ok = false;
    }
    void tm_reset() { tm_free(); tm_active = false; tm_mask.clear(); tm_cnt.clear(); tm_gid.clear(); tm_ntrain = 0; tm_ngroups = 0; tm_enc_frozen = false; tm_last_step = 0; }
    // index of the bound tensor that holds flat offset `off` (-1: padding / outside)
    int tensor_at(int64_t off) const {
        for (size_t t = 0; t < gn_tens.size(); ++t) if (off >= gn_tens[t].off && off < gn_tens[t].off + gn_tens[t].n) return (int)t;
        return -1;
    }
    bool tm_trainable_at(int64_t off) const { const int t = tensor_at(off); return t < 0 || tm_mask[t] != 0; }
    bool tm_trainable_w(const float* w32) const { return !w32 || tm_trainable_at(w32 - P); }
    // the tensor a transpose descriptor reads: a view of the parameters (fp32 engine) / of their 16-bit shadow, or one of the two packed sources
    int desc_tensor(const TrDesc& d) const {
        if (d.src == (const void*)encG.fc7.W && encG.fc7.own_w) return tensor_at(encG.fc7.W32 - P);
        if (std::is_same<T, float>::value) { const float* s = (const float*)d.src; return (s >= P && s < P + numel) ? tensor_at(s - P) : -1; }
        const T* s = (const T*)d.src;
        return (wshadow && s >= wshadow && s < wshadow + numel) ? tensor_at(s - wshadow) : -1;
    }
    bool heads_trainable() const { for (int i = 0; i < 4; ++i) if ((head_w32[i] && tm_trainable_w(head_w32[i])) || (head_b32[i] && tm_trainable_w(head_b32[i]))) return true; return false; }
    bool desc_trainable(const TrDesc& d) const {
        if (d.src == (const void*)wheads) return heads_trainable();
        const int t = desc_tensor(d);
        return t < 0 || tm_mask[t] != 0;
    }
    bool range_all_frozen(int64_t lo, int64_t hi) const {
        if (!tm_active) return false;
        for (size_t t = 0; t < gn_tens.size(); ++t) if (gn_tens[t].off >= lo && gn_tens[t].off < hi && tm_mask[t]) return false;
        return true;
    }
    // count of optimizer steps taken so far: the device-side count under the loss scaler (a skipped step is nobody's step), else the caller's
    int steps_now(int64_t* out) {
        if (!scaler) { *out = tm_last_step; return 0; }
        ScalerState h;
        HIP_CHECK(hipMemcpyAsync(&h, scaler, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        *out = h.steps;
        return 0;
    }
    int tm_commit(const char* who, const std::vector<uint8_t>& mask, const std::vector<int64_t>& cnt) {
        static_assert(OPT_GROUPS == hulc_trainable::MAX_GROUPS, "kernels.h OptGroups holds one slot per group of trainable_plan.h");
        std::vector<int64_t> offs;
        char msg[256];
        if (hulc_trainable::plan_groups(who, mask, cnt, offs, msg, sizeof(msg))) { hulc_set_error("%s", msg); return 1; }      // nothing has changed yet
        tm_mask = mask; tm_cnt = cnt; tm_active = true;
        tm_ngroups = (int)offs.size();
        for (int g = 0; g < OPT_GROUPS; ++g) tm_goff[g] = g < tm_ngroups ? offs[g] : 0;
        tm_gid.assign(mask.size(), 0);
        tm_ntrain = 0;
        for (size_t t = 0; t < mask.size(); ++t) if (mask[t]) { ++tm_ntrain; tm_gid[t] = (uint8_t)(std::find(offs.begin(), offs.end(), cnt[t]) - offs.begin()); }
        return tm_build(who);
    }
    int tm_build(const char* who) {
        HIP_CHECK(hipStreamSynchronize(st));      // a step still in flight reads the tables that are freed here
        tm_free();
        std::vector<int> all, comp;
        for (size_t t = 0; t < tm_mask.size(); ++t) if (tm_mask[t]) all.push_back((int)t);
        // tiles: the trainable matrices of the optimizer's tile pass; complement: every other trainable tensor
        std::vector<TrDesc> tiles; std::vector<unsigned char> tg; std::vector<uint8_t> tiled(tm_mask.size(), 0);
        tm_tile_ok = !tr_fused_host.empty();
        for (const TrDesc& d : tr_fused_host) {
            const int t = desc_tensor(d);
            const int64_t off = (const T*)d.src - wshadow;
            if (t < 0 || gn_tens[t].off != off || gn_tens[t].n != (int64_t)d.R * d.C || tiled[t]) { tm_tile_ok = false; break; }
            tiled[t] = 1;
            if (tm_mask[t]) { tiles.push_back(d); tg.push_back(tm_gid[t]); }
        }
        if (!tm_tile_ok) tiles.clear();
        for (int t : all) if (!tm_tile_ok || !tiled[t]) comp.push_back(t);
        std::vector<TrDesc> tr_all, tr_rest_m;
        for (const TrDesc& d : trdesc) if (desc_trainable(d)) tr_all.push_back(d);
        for (const TrDesc& d : tr_rest_host) if (desc_trainable(d)) tr_rest_m.push_back(d);
        bool ok = chunk_table_build(tm_flat, all) && chunk_table_build(tm_comp, comp) && tr_table_build(tm_tiles, tiles) && tr_table_build(tm_tr_all, tr_all) &&
                  tr_table_build(tm_tr_rest, tr_rest_m);
        if (ok && !tg.empty()) {
            ok = hipMalloc((void**)&tm_tile_gid, tg.size()) == hipSuccess;
            if (ok) hipMemcpy(tm_tile_gid, tg.data(), tg.size(), hipMemcpyHostToDevice);
        }
        if (!ok) { tm_free(); hulc_set_error("%s: allocation of the optimizer tables failed", who); return 1; }
        // fragment-ordered copies: jobs come in pairs (W, then W^T whose source is the transposed copy): a pair follows its weight
        for (int i = 0; i + 1 < fragbatch.n; i += 2) {
            const T* s = (const T*)fragbatch.src[i];
            if (wshadow && s >= wshadow && s < wshadow + numel && !tm_trainable_at(s - wshadow)) continue;
            for (int u = 0; u < 2; ++u) {
                const int k = tm_frag.n;
                tm_frag.src[k] = fragbatch.src[i + u]; tm_frag.dst[k] = fragbatch.dst[i + u]; tm_frag.N[k] = fragbatch.N[i + u]; tm_frag.K[k] = fragbatch.K[i + u];
                tm_frag.blk0[k] = tm_frag_blocks; tm_frag_blocks += frag_pack_blocks(tm_frag.N[k], tm_frag.K[k]); ++tm_frag.n;
            }
            tm_frag.blk0[tm_frag.n] = tm_frag_blocks;
        }
        tm_enc_frozen = false;
        { bool any = false, allf = true;
          for (size_t t = 0; t < tm_mask.size(); ++t) if (tm_names[t].compare(0, 19, "perceptual_encoder.") == 0) { any = true; if (tm_mask[t]) allf = false; }
          tm_enc_frozen = any && allf; }
        // data parallelism: the skip vote rides in a padding element of a bucket that is still reduced and issued behind every recurrence — the encoders' bucket,
        // else the goal encoders'; with both frozen it travels as a word of its own (engine_backward.inc vote_only)
        if (bucket_plan_ok()) {
            const std::vector<Bucket> v = bucket_plan();
            skip_pad = -1;
            for (int b : {4, 3}) {
                if (skip_pad >= 0 || b >= (int)v.size() || v[b].hi <= v[b].lo || range_all_frozen(v[b].lo, v[b].hi)) continue;
                for (size_t i = 0; i < tab_order.size(); ++i) {
                    const Ref& r = tab_order[i].second;
                    const int64_t end = r.off + r.n, nxt = i + 1 < tab_order.size() ? tab_order[i + 1].second.off : numel;
                    if (r.off >= v[b].lo && r.off < v[b].hi && end < nxt && end < numel) { skip_pad = end; break; }
                }
            }
        }
        return gn_build();      // the norm pass (and the fp16 non-finite check that rides on it) lists the trainable tensors only; a frozen tensor reports 0
    }

    int trainable_set(int32_t n, const uint8_t* trainable) override {
        char msg[256];
        if (ema_refuse("hulc_trainable_set")) return 1;
        if (hulc_trainable::check_call("hulc_trainable_set", bound, (long long)gn_tens.size(), n, msg, sizeof(msg))) { hulc_set_error("%s", msg); return 1; }
        int64_t taken = 0;
        if (steps_now(&taken)) return 1;
        std::vector<uint8_t> mask = tm_active ? tm_mask : std::vector<uint8_t>(gn_tens.size(), 1);
        std::vector<int64_t> cnt = tm_active ? tm_cnt : std::vector<int64_t>(gn_tens.size(), 0);
        hulc_trainable::apply_mask(trainable, taken, mask, cnt);
        return tm_commit("hulc_trainable_set", mask, cnt);
    }
    int trainable_get(int64_t cap, uint8_t* trainable_out, int64_t* frozen_steps_out) override {
        if (!bound) { hulc_set_error("hulc_trainable_get before hulc_bind_params"); return 1; }
        const int64_t n = (int64_t)gn_tens.size();
        if (cap < n) { hulc_set_error("hulc_trainable_get: the buffers hold %lld entries, %lld tensors are bound", (long long)cap, (long long)n); return 1; }
        int64_t taken = 0;
        if (tm_active && steps_now(&taken)) return 1;
        for (int64_t t = 0; t < n; ++t) {
            if (trainable_out) trainable_out[t] = tm_active ? tm_mask[t] : 1;
            if (frozen_steps_out) frozen_steps_out[t] = !tm_active ? 0 : hulc_trainable::frozen_steps(tm_mask[t], tm_cnt[t], taken);
        }
        return 0;
    }
    int trainable_steps_set(int32_t n, const int64_t* frozen_steps, int64_t steps_taken) override {
        char msg[256];
        if (hulc_trainable::check_call("hulc_trainable_steps_set", bound, (long long)gn_tens.size(), n, msg, sizeof(msg))) { hulc_set_error("%s", msg); return 1; }
        int64_t taken = steps_taken;
        if (taken < 0 && steps_now(&taken)) return 1;
        for (int t = 0; t < n; ++t)
            if (frozen_steps[t] < 0 || frozen_steps[t] > taken) { hulc_set_error("hulc_trainable_steps_set: tensor %d sat out %lld of %lld optimizer steps", t, (long long)frozen_steps[t], (long long)taken); return 1; }
        std::vector<uint8_t> mask = tm_active ? tm_mask : std::vector<uint8_t>(gn_tens.size(), 1);
        std::vector<int64_t> cnt(gn_tens.size());
        for (int t = 0; t < n; ++t) cnt[t] = mask[t] ? frozen_steps[t] : taken - frozen_steps[t];
        const int rc = tm_commit("hulc_trainable_steps_set", mask, cnt);
        if (!rc && !scaler) tm_last_step = taken;
        return rc;
    }
