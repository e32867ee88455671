// hulc_amd/csrc/engine_ema.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body: the averaged weights
// (hulc_ema_enable / hulc_ema_state_get / hulc_ema_state_set / hulc_ema_swap / hulc_ema_swapped).  Not a standalone header.
//
// A context that never enables the average keeps `ema == nullptr` and launches what it always launched.  With it on, the optimizer step enqueues
// ema_update_kernel + ema_count_kernel (kernels.h) between the optimizer kernel and scaler_update_kernel: the whole flat buffer, or the trainable mask's chunk
// table (tm_flat), so that the average of a frozen tensor is neither read nor written.  hulc_ema_swap exchanges the parameter buffer with the average and
// rebuilds every weight copy from it; until the swap back, whatever would write the parameters or the gradients is refused before any launch.
    float* ema = nullptr;                 // borrowed, numel fp32 in the layout of P; null = off
    EmaState* ema_state = nullptr;        // device
    EmaState ema_cfg{};                   // host mirror of decay / start_step / warmup (updates lives on the device only)
    bool ema_swapped = false;

    // true (and the message) while the averaged weights stand in the parameter buffer
    bool ema_refuse(const char* who) {
        if (!ema_swapped) return false;
        hulc_set_error("%s: the averaged weights are swapped in (hulc_ema_swap back first)", who);
        return true;
    }
    // behind the optimizer kernel of step `tag`, before scaler_update_kernel clears found_inf
    void ema_step(unsigned tag) {
        if (!tm_active) launch_ema_update(st, ema, P, (long long)numel, ema_state, 0.f, nullptr, nullptr, 0, scaler, rp_skip, tag);
        else if (tm_flat.chunks) launch_ema_update(st, ema, P, (long long)numel, ema_state, 0.f, tm_flat.start, tm_flat.n, tm_flat.chunks, scaler, rp_skip, tag);
        hipLaunchKernelGGL(ema_count_kernel, dim3(1), dim3(1), 0, st, ema_state, (const ScalerState*)scaler, (const unsigned*)rp_skip, tag);
    }
    int ema_state_write(const EmaState& h) {
        HIP_CHECK(hipMemcpyAsync(ema_state, &h, sizeof(h), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));          // `h` lives on the caller's frame
        return 0;
    }
    int ema_enable(float* buf, float decay, int64_t start_step, int32_t warmup) override {
        if (!bound) { hulc_set_error("hulc_ema_enable before hulc_bind_params"); return 1; }
        if (ema_refuse("hulc_ema_enable")) return 1;
        if (!buf) { ema = nullptr; return 0; }
        if (!(decay > 0.f && decay < 1.f) || start_step < 0) { hulc_set_error("hulc_ema_enable: need 0 < decay < 1 and start_step >= 0 (got %g, %lld)", (double)decay, (long long)start_step); return 1; }
        if (reinterpret_cast<uintptr_t>(buf) & 15) { hulc_set_error("hulc_ema_enable: the buffer must be 16-byte aligned"); return 1; }
        if (!ema_state) { ema_state = alloc<EmaState>(1); if (alloc_failed) { ema_state = nullptr; hulc_set_error("hulc_ema_enable: allocation failed"); return 1; } }
        EmaState h{}; h.updates = 0; h.decay = decay; h.start_step = start_step; h.warmup = warmup != 0;
        HIP_CHECK(hipMemcpyAsync(buf, P, sizeof(float) * numel, hipMemcpyDeviceToDevice, st));      // the average starts from the current parameters
        if (ema_state_write(h)) return 1;
        ema_cfg = h; ema = buf;
        return 0;
    }
    int ema_state_get(int64_t* updates, float* last_decay) override {
        if (!ema) { hulc_set_error("hulc_ema_state_get: the average is off (hulc_ema_enable first)"); return 1; }
        EmaState h;
        HIP_CHECK(hipMemcpyAsync(&h, ema_state, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (updates) *updates = h.updates;
        // 0 before the first update and through the copy phase (e = p is decay 0)
        if (last_decay) *last_decay = (h.updates < 1 || h.updates < h.start_step) ? 0.f : ema_decay_of(h.updates, h.decay, h.warmup);
        return 0;
    }
    int ema_state_set(int64_t updates) override {
        if (!ema) { hulc_set_error("hulc_ema_state_set: the average is off (hulc_ema_enable first)"); return 1; }
        if (updates < 0) { hulc_set_error("hulc_ema_state_set: updates %lld is negative", (long long)updates); return 1; }
        EmaState h = ema_cfg; h.updates = updates;
        return ema_state_write(h);
    }
    int ema_swap() override {
        if (!ema) { hulc_set_error("hulc_ema_swap: the average is off (hulc_ema_enable first)"); return 1; }
        if (bwd_stage != 0) { hulc_set_error("hulc_ema_swap: encoder part of the backward still pending"); return 1; }
        hipLaunchKernelGGL(ema_swap_kernel, dim3(2048), dim3(256), 0, st, P, ema, (long long)numel);
        if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_ema_swap: launch failed"); return 1; }
        ema_swapped = !ema_swapped;
        // what was computed from the other weights goes: the activations a backward would read, the B = 1 rollout state and every rollout slot (the slots
        // cache a decoder input term)
        have_fwd = false;
        rollout_reset();
        if (env_max >= 1 && rollout_envs_reset(0, nullptr, 0)) return 1;
        return prepare_weights(false);      // the full form: the shadow is recast from P, every copy refreshed, frozen tensors included
    }
    int ema_is_swapped(int32_t* out) override { if (out) *out = ema_swapped ? 1 : 0; return 0; }
