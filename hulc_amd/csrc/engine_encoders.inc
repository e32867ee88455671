// hulc_amd/csrc/engine_encoders.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body; not a standalone header.
// The perceptual encoders (SURVEY 8 a3-a6): where conv1 reads its frames (conv1_src: fp32 / uint8 / frame store / variable-length windows), then the driver of the
// forward and backward pass.  The driver is a list of stages (enc_fwd_stages, enc_bwd_stages).  Each stage has a single-camera function (conv1_fwd, conv_fwd, head_fwd;
// head_bwd, conv_dgrad) and, where the 16-bit engines run both cameras as jobs of one launch, a *_both function that returns false when it
// launched nothing; the list then calls the single-camera function once per camera.  The weight-gradient stages (conv_wgrad, conv1_wgrad) are one function each over
// the camera range: the joint launch when the range holds both cameras, else per camera.  Weight-gradient slabs are queued (queue_unpack) and reduced by one launch
// (flush_unpacks).  The rest of the engine calls conv1_src / conv1_src_f32, window_tables (+ enc_frames, ragged: the ragged encoder pass), store_args_bad, actions_of, enc_fwd_both, enc_tail_fusable,
// enc_tail_fwd_both, enc_tail_bwd_both, enc_bwd_both and flush_unpacks.
    ConvGeom geom(int Nf, int IH, int C, int K, int S) const {
        ConvGeom g; g.Nf = Nf; g.IH = g.IW = IH; g.C = C; g.KH = g.KW = K; g.S = S; g.OH = g.OW = (IH - K) / S + 1; return g;
    }
    // conv1 input of the current batch: the reference's fp32 NCHW frames, or uint8 NHWC frames + the fused dataloader transforms
    Conv1Src conv1_src(const hulc_batch& b, bool gripper) const {
        Conv1Src s;
        s.X = gripper ? b.rgb_gripper : b.rgb_static;
        s.u8 = b.frames_u8 != 0;
        s.shift = s.u8 ? (gripper ? b.shift_gripper : b.shift_static) : nullptr;
        s.pad = gripper ? b.pad_gripper : b.pad_static;
        // 16-bit engines: the dataloader's affine is folded out of the uint8 data path (conv1_stage.h Conv1Src::fold); the fp32 (parity) engine converts
        // exactly like the reference (ingest_u8_kernel)
        s.fold = (s.u8 && std::is_same<T, h16_t>::value && u8_fold_mode) ? 1 : 0;
        if (s.u8 && b.window_start) { s.wstart = reinterpret_cast<const long long*>(b.window_start); s.S = b.S; s.nstore = b.store_frames; }      // windows gathered from the frame store
        if (s.wstart && (b.window_len || b.window_len_host)) {      // variable-length padded windows: the per-frame table of window_len_expand (ragged pass: the compact table of window_tables), read as one-frame windows
            const int set = &b == &cur2 ? 1 : 0;
            s.wstart = wl_frame[set]; s.S = 1;
            if (s.shift) s.shift = wl_shift[set][gripper ? 1 : 0];
        }
        return s;
    }
    // fp32 NCHW frames read as they are (the rollout's observations): no dataloader transform, no frame store
    static Conv1Src conv1_src_f32(const void* x) { return Conv1Src{x, nullptr, 0, 0}; }
    // hulc_batch::window_len, expanded once per forward / validation (window_rows.h window_expand_kernel); set 0 = the batch of the pass, 1 = the paired pass's lang batch (cur2)
    long long* wl_frame[2] = {nullptr, nullptr};
    int* wl_shift[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int wl_alloc(int set) {
        if (!wl_frame[set]) {
            wl_frame[set] = alloc<long long>((int64_t)maxN); wl_shift[set][0] = alloc<int>((int64_t)maxN * 2); wl_shift[set][1] = alloc<int>((int64_t)maxN * 2);
            if (alloc_failed) { hulc_set_error("window_len: workspace allocation failed"); return 1; }
        }
        return 0;
    }
    int window_len_expand(const hulc_batch& b, int nB, int set) {
        if (!b.window_len) return 0;
        if (wl_alloc(set)) return 1;
        hipLaunchKernelGGL(window_expand_kernel, dim3(cdiv(nB * b.S, 256)), dim3(256), 0, st, reinterpret_cast<const long long*>(b.window_start), b.window_len, nB, b.S,
                           (long long)b.store_frames, b.shift_static, b.shift_gripper, wl_frame[set], wl_shift[set][0], wl_shift[set][1]);
        return 0;
    }
    // ---- ragged encoder pass (hulc_batch::window_len_host): the encoders run on the N' real frames of the pass, their output is expanded to the (B,S,EMB) rows the
    // rest of the engine reads (rows_expand_kernel) and the embedding gradient is reduced to compact rows before the encoder backward (rows_reduce_kernel).
    // rg_host / rg_dev: [off (nJ + 1) | lens (nJ)] over the nJ windows of the pass (the paired pass: vis then lang), clamped and summed on the host — every table,
    // grid and frame count below comes from this one array.  rg_n1 = the frames of the first conv1 source (the whole pass unless paired), rg_N = N'.
    // The state of a pass is cur.window_len_host (ragged()): the rollout paths set cur to a zeroed batch.
    std::vector<int> rg_host;
    int* rg_dev = nullptr;
    T* emb_c = nullptr; float* demb_c = nullptr;
    int rg_nJ = 0, rg_n1 = 0, rg_N = 0;
    long long enc_frames_last = 0;
    bool ragged() const { return cur.window_len_host != nullptr; }
    const int* rg_off() const { return rg_dev; }
    const int* rg_lens() const { return rg_dev + rg_nJ + 1; }
    int enc_frames(int N) const { return ragged() ? rg_N : N; }      // the frame count of the encoder stages of this pass
    T* enc_emb() { return ragged() ? emb_c : emb; }                  // where the encoders' tails write / read their rows
    float* enc_demb() { return ragged() ? demb_c : demb; }
    // frames of conv1 source h of a two-source (paired) pass over Nf frames
    int src_frames(int Nf, int h) const { return ragged() ? (h ? Nf - rg_n1 : rg_n1) : Nf / 2; }
    // the per-frame tables of the pass, once per forward / validation: b (nB windows) and, in the paired pass, b2
    int window_tables(const hulc_batch& b, int nB, const hulc_batch* b2) {
        if (!b.window_len_host) return (window_len_expand(b, nB, 0) || (b2 && window_len_expand(*b2, b2->B, 1))) ? 1 : 0;
        const int nJ = nB + (b2 ? b2->B : 0);
        if (!rg_dev) { rg_dev = alloc<int>((int64_t)2 * maxB + 1); emb_c = alloc<T>((int64_t)maxN * EMB); demb_c = alloc<float>((int64_t)maxN * EMB); }
        if (alloc_failed || wl_alloc(0) || (b2 && wl_alloc(1))) { hulc_set_error("window_len_host: workspace allocation failed"); return 1; }
        rg_host.resize((size_t)2 * nJ + 1);
        int *off = rg_host.data(), *len = off + nJ + 1;
        off[0] = 0;
        for (int i = 0; i < nJ; ++i) {
            const hulc_batch& s = i < nB ? b : *b2;
            const int lmax = (int)std::min<long long>(s.S, s.store_frames);
            len[i] = std::min(std::max(s.window_len_host[i < nB ? i : i - nB], 1), lmax);
            off[i + 1] = off[i] + len[i];
        }
        rg_nJ = nJ; rg_n1 = off[nB]; rg_N = off[nJ];
        HIP_CHECK(hipMemcpyAsync(rg_dev, rg_host.data(), sizeof(int) * rg_host.size(), hipMemcpyHostToDevice, st));
        launch_window_compact(st, reinterpret_cast<const long long*>(b.window_start), rg_lens(), rg_off(), 0, nB, b.S, (long long)b.store_frames, b.shift_static, b.shift_gripper,
                              wl_frame[0], wl_shift[0][0], wl_shift[0][1]);
        if (b2) launch_window_compact(st, reinterpret_cast<const long long*>(b2->window_start), rg_lens() + nB, rg_off() + nB, rg_n1, b2->B, b2->S, (long long)b2->store_frames,
                                      b2->shift_static, b2->shift_gripper, wl_frame[1], wl_shift[1][0], wl_shift[1][1]);
        return 0;
    }
    // argument check of the frame-store fields, before any launch (hulc_forward_loss / _pair, hulc_validate): true = error set
    static bool store_args_bad(const hulc_batch* b) {
        if (b->window_len && !b->window_start) { hulc_set_error("window_len (variable-length windows) needs window_start (the frame store)"); return true; }
        if (b->window_len_host && !b->window_start) { hulc_set_error("window_len_host (ragged encoder pass) needs window_start (the frame store)"); return true; }
        if (!b->window_start) return false;
        if (b->store_frames < 1) { hulc_set_error("window_start (frame store) needs store_frames >= 1 (got %lld)", (long long)b->store_frames); return true; }
        // fixed windows need S frames in the store; with window_len a window may be as short as one frame
        if (!b->frames_u8 || (!b->window_len && !b->window_len_host && b->store_frames < b->S)) { hulc_set_error("window_start (frame store) needs frames_u8 and store_frames >= S (got frames_u8=%d, store_frames=%lld, S=%d)", b->frames_u8, (long long)b->store_frames, b->S); return true; }
        return false;
    }
    // b - sum_k W16 of the two conv1 layers (Conv1Src::fold), recomputed after every weight refresh, only when a uint8 batch asks for it
    float* c1_bias_fold[2] = {nullptr, nullptr};
    bool c1_bias_fold_valid = false;
    const float* conv1_bias(const EncW& e, const Conv1Src& src) {
        if (!src.fold) return e.c1.b32;
        if constexpr (std::is_same<T, h16_t>::value) {
            if (!c1_bias_fold[0]) { c1_bias_fold[0] = alloc<float>(64); c1_bias_fold[1] = alloc<float>(64); }
            if (!c1_bias_fold_valid) {
                hipLaunchKernelGGL(conv1_bias_fold_kernel, dim3(32), dim3(64), 0, st, encS.c1.Wf, encS.c1.b32, c1_bias_fold[0]);
                hipLaunchKernelGGL(conv1_bias_fold_kernel, dim3(32), dim3(64), 0, st, encG.c1.Wf, encG.c1.b32, c1_bias_fold[1]);
                c1_bias_fold_valid = true;
            }
            return c1_bias_fold[e.gripper ? 1 : 0];
        }
        return e.c1.b32;
    }
    // actions of the current batch: the reference's relative actions, or absolute targets + RelativeActions applied here
    float* act_rel = nullptr;
    const float* actions_of(const hulc_batch& b) {
        if (!b.actions_absolute) return b.actions;
        if (!act_rel) act_rel = alloc<float>((int64_t)maxN * 7);
        hipLaunchKernelGGL(relative_actions_kernel, dim3(cdiv(b.B * b.S, 256)), dim3(256), 0, st, b.actions, b.robot_obs, b.B * b.S, b.max_rel_pos, b.max_rel_orn, act_rel);
        return act_rel;
    }
    float* x32[2] = {nullptr, nullptr};       // fp32 (parity) mode + uint8 ingest: the transformed frames are materialised once per step
    const float* conv1_f32(const Conv1Src& src, bool gripper, int Nf, int IH, long long frame_off = 0) {
        if (!src.u8) return reinterpret_cast<const float*>(src.X);
        float*& buf = x32[gripper ? 1 : 0];
        if (!buf) buf = alloc<float>((int64_t)maxN * 3 * IH * IH);
        const long long n = (long long)Nf * 3 * IH * IH;
        float* dst = buf + frame_off * 3 * IH * IH;
        hipLaunchKernelGGL(ingest_u8_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(src.X), src.shift, src.pad, Nf, IH, IH, dst, src);
        return dst;
    }
    // ---- paired pass (vis + lang windows of one step as ONE 2B-window pass, hulc_forward_loss_pair): rows [0, pairBv) are the vis
    // windows, the rest the lang windows; frames (and their shifts) stay in the two batches' own buffers, everything else is joint
    bool pair = false; int pairBv = 0; hulc_batch cur2;
    float *act_j = nullptr, *ro_j = nullptr, *eps_j = nullptr, *losses2 = nullptr; int* aux_j = nullptr;

    // ---- the stages of one camera.  Camera k: 0 = static, 1 = gripper; its embedding columns are [64 k, 64 k + 64).  Everything a camera owns (weights, activations,
    // gradient buffers) hangs off encw(k) / enca(k): no stage picks a buffer by camera.
    const EncW& encw(int k) const { return k ? encG : encS; }
    EncA& enca(int k) { return k ? aG : aS; }
    // conv2 (sn == 2) or conv3 (sn == 3) of camera k on Nf frames: the layer, its geometry, input x and output y, their gradients, the ReLU bit masks of x and y
    struct Stage { const ConvW& c; ConvGeom g; T *x, *y, *dx, *dy; unsigned *xbits, *ybits; };
    Stage stage(int k, int sn, int Nf) {
        const EncW& e = encw(k); EncA& a = enca(k);
        if (sn == 3) return Stage{e.c3, geom(Nf, e.H2, 64, 3, 1), a.a2, a.a3, a.dact2, a.dact3, a.m2bits, nullptr};
        return Stage{e.c2, geom(Nf, e.H1, 32, 4, 2), a.a1, a.a2, a.dact1, a.dact2, a.m1bits, a.m2bits};
    }
    // what the timers account for a launch (SURVEY 8(d): algorithmic bytes, every operand once).  xbytes: bytes per element of the layer's input as the weight
    // gradient reads it (16-bit activations: 2; conv1's frames: 1 as uint8, 4 as fp32)
    static double conv_fwd_flops(const ConvW& c, const ConvGeom& g) { return 2.0 * g.Nf * g.OH * g.OW * c.O * c.I * c.KH * c.KW; }
    static double conv_fwd_bytes(const ConvW& c, const ConvGeom& g) { return ((double)g.Nf * g.IH * g.IW * c.I + (double)g.Nf * g.OH * g.OW * c.O) * 2; }
    static double conv_wgrad_flops(const ConvW& c, const ConvGeom& g) { return 2.0 * g.Nf * g.OH * g.OW * c.O * c.I * c.KH * c.KW; }
    static double conv_wgrad_bytes(const ConvW& c, const ConvGeom& g, int xbytes) { return (double)g.Nf * g.IH * g.IW * c.I * xbytes + (double)g.Nf * g.OH * g.OW * c.O * 2; }

    float* pend_zero[2] = {nullptr, nullptr};   // loss accumulators the next conv1 forward launch clears (16-bit engines)
    // conv1 forward of one camera.  Paired pass (src2): the first src_frames(Nf, 0) frames (Nf/2; the ragged pass: the vis batch's N') come from src, the rest from
    // src2 — one launch per source, the later stages run on all Nf frames
    void conv1_fwd(int k, const Conv1Src& src, int Nf, const Conv1Src* src2) {
        const EncW& e = encw(k); EncA& a = enca(k);
        for (int h = 0; h < (src2 ? 2 : 1); ++h) {
            const int nf = src2 ? src_frames(Nf, h) : Nf;
            const ConvGeom g = geom(nf, e.IH, 3, 8, 4);
            const Conv1Src& sh = h ? *src2 : src;
            const long long foff = h ? src_frames(Nf, 0) : 0, poff = foff * g.OH * g.OW;
            if constexpr (std::is_same<T, h16_t>::value) {
                const double px = (double)nf * g.OH * g.OW;
                TimerScope ts(this, "conv1_fwd", "hbm", 2.0 * px * 32 * 192, (double)nf * 3 * e.IH * e.IH * (sh.u8 ? 1 : 4) + px * 32 * 2);
                launch_conv1_fwd(st, sh, e.c1.Wf, conv1_bias(e, sh), a.a1 + poff * 32, nf, e.IH, e.IH, g.OH, g.OW, false, a.m1bits ? a.m1bits + poff : nullptr, pend_zero[0], pend_zero[1]);
                pend_zero[0] = pend_zero[1] = nullptr;
            } else {
                const float* x = conv1_f32(sh, e.gripper, nf, e.IH, foff);
                Conv1Loader<T> l{x, g};
                EpiP ep = epi(a.a1 + poff * 32, false); ep.bias = e.c1.b32; ep.relu = 1;
                launch_gemm<T, 128, 32>(st, l, dense<T>(e.c1.Wf, 32, 192), dense_out(32), ep, nf * g.OH * g.OW, 32, 192);
            }
        }
    }
    ConvTileP conv_fwd_job(const Stage& s) const {
        ConvTileP p{}; p.img = s.x; p.IMH = p.IMW = s.g.IH; p.w = s.c.Wf; p.out = s.y; p.OUTH = p.OUTW = s.g.OH; p.bias = s.c.b32; p.relu = 1; p.Nf = s.g.Nf; p.bits_out = s.ybits;
        return p;
    }
    // conv2 / conv3 forward of one camera.  16-bit engines: the weights-in-registers kernels (conv_reg.h) — large maps (the static camera) take the one-workgroup form
    // with the band-invariant DMA slot decode held in registers (PKR), the gripper camera's stacked small maps the form with two co-resident 256-thread workgroups per
    // CU (NWV = 4) — then the raw-tile kernels (conv_tile.h: weights resident in LDS, bands streamed once).  The implicit GEMM is the fp32 engine's form and the last resort
    void conv_fwd(int k, int sn, int Nf) {
        const Stage s = stage(k, sn, Nf);
        if constexpr (std::is_same<T, h16_t>::value) {
            const ConvTileP p = conv_fwd_job(s);
            const bool big = encw(k).H2 >= 16;
            TimerScope ts(this, "conv_tile_fwd", "mfma", conv_fwd_flops(s.c, s.g), conv_fwd_bytes(s.c, s.g));
            if (sn == 2 ? (big ? launch_conv_reg_fwd<32, 4, 4, 2>(st, p) : launch_conv_reg<32, 4, 4, 2, false, 1, 4, true>(st, p)) || launch_conv_tile<32, 64, 4, 4, 2, 1, false>(st, p)
                        : (big ? launch_conv_reg_fwd<64, 3, 3, 1>(st, p) : launch_conv_reg<64, 3, 3, 1, false, 1, 4>(st, p)) || launch_conv_tile<64, 64, 3, 3, 1, 1, false>(st, p)) return;
        }
        const int Kc = s.c.I * s.c.KH * s.c.KW;
        ConvNHWCLoader<T> l{s.x, s.g};
        EpiP ep = epi(s.y, false); ep.bias = s.c.b32; ep.relu = 1;
        launch_gemm<T, 128, 64>(st, l, dense<T>(s.c.Wf, 64, Kc), dense_out(64), ep, Nf * s.g.OH * s.g.OW, 64, Kc);
    }
    // what follows conv3 in one camera: spatial softmax (static) or fc7 (gripper), then the dense tail unless both cameras' tails run as one launch (enc_tail_fwd_both)
    void head_fwd(int k, int Nf, bool defer_tail) {
        const EncW& e = encw(k); EncA& a = enca(k);
        const T* fin;
        if (!e.gripper) {
            if constexpr (std::is_same<T, h16_t>::value) launch_spatial_softmax64_fwd(st, a.a3, Nf, e.H3, e.H3, a.ss, a.ssstats);
            else hipLaunchKernelGGL((spatial_softmax_fwd_kernel<T>), dim3(Nf), dim3(256), 0, st, a.a3, e.H3, e.H3, 64, a.ss, (float*)nullptr, a.ssstats);
            fin = a.ss;
        } else {
            EpiP ep = epi(a.g0, false); ep.relu = 1;
            lin_fwd(a.a3, 3136, Nf, e.fc7, ep, 128);
            fin = a.g0;
        }
        if (defer_tail) return;
        { EpiP ep = epi(a.f1, false); ep.relu = 1; lin_fwd(fin, 128, Nf, e.fc1, ep, 512); }
        { EpiP ep = epi(a.f2, true); lin_fwd(a.f1, 512, Nf, e.fc2, ep, 64); }
        ln_fwd(a.f2, 64, Nf, 64, e.lng, e.lnb, enc_emb() + k * 64, EMB, nullptr, 0, a.lnst);
    }
    // conv2 / conv3 forward of BOTH cameras as one launch (conv_reg.h launch_conv_reg_jobs): the gripper camera's job runs in the static camera's 8-wave form on its
    // share of the persistent workgroups, its prologue and tail under the static job's throughput.  false = nothing launched (shape-decided); the timer accounts
    // only a launch that was taken — what falls back accounts for itself
    bool conv_fwd_both(int sn, int Nf) {
        if constexpr (std::is_same<T, h16_t>::value) {
            const Stage S = stage(0, sn, Nf), G = stage(1, sn, Nf);
            const ConvTileP j[2] = {conv_fwd_job(S), conv_fwd_job(G)};
            TimerScope ts(this, "conv_tile_fwd", "mfma", 0, 0, 0);
            const bool ok = sn == 2 ? launch_conv_reg_fwd_jobs<32, 4, 4, 2>(st, j, 2) : launch_conv_reg_fwd_jobs<64, 3, 3, 1>(st, j, 2);
            if (ok) ts.add(conv_fwd_flops(S.c, S.g) + conv_fwd_flops(G.c, G.g), conv_fwd_bytes(S.c, S.g) + conv_fwd_bytes(G.c, G.g));
            return ok;
        }
        return false;
    }
    // The encoders' forward of cameras [k0, k1) as a list of stages: a stage is the two-camera launch where there is one and it takes the shape, else the
    // single-camera function once per camera.  The two networks are independent; the 16-bit engines run both cameras through one list.  The fp32 engine has no
    // two-camera launch and one set of gradient buffers for both cameras (alloc_all), so it runs the list once per camera.
    void enc_fwd_stages(int k0, int k1, const Conv1Src* src, const Conv1Src* src2, int Nf, bool defer_tail) {
        const bool both = k1 - k0 == 2;
        for (int k = k0; k < k1; ++k) conv1_fwd(k, src[k], Nf, src2 ? &src2[k] : nullptr);
        for (int sn = 2; sn <= 3; ++sn)
            if (!(both && conv_fwd_both(sn, Nf))) for (int k = k0; k < k1; ++k) conv_fwd(k, sn, Nf);
        for (int k = k0; k < k1; ++k) head_fwd(k, Nf, defer_tail);
    }
    // src[2], src2[2] (paired pass, else null): the conv1 sources of the static and the gripper camera
    void enc_fwd_both(const Conv1Src* src, const Conv1Src* src2, int Nf, bool defer_tail) {
        if constexpr (std::is_same<T, h16_t>::value) enc_fwd_stages(0, 2, src, src2, Nf, defer_tail);
        else for (int k = 0; k < 2; ++k) enc_fwd_stages(k, k + 1, src, src2, Nf, defer_tail);
    }
    // enc_tail.h is written for the reference's tail widths (128 -> 512 -> 64, vision_network.py:46-52 / vision_network_gripper.py:18-27) and EMB = 2 x 64
    bool enc_tail_fusable() const {
        if constexpr (!std::is_same<T, h16_t>::value) return false;
        auto ok = [](const EncW& e) { return e.fc1.K == 128 && e.fc1.N == 512 && e.fc2.K == 512 && e.fc2.N == 64; };
        return ok(encS) && ok(encG) && EMB == 128;
    }
    // fc1 + ReLU, fc2 and the LayerNorm of both encoders in one launch (enc_tail.h)
    // with_x0: the same launch also writes the plan-recognition transformer's input (enc_tail.h) — pr_fwd then skips its posadd launch
    bool x0_done = false;
    void enc_tail_fwd_both(int Nf, bool with_x0 = false, int S = 1, float dp = 0.f) {
        if constexpr (std::is_same<T, h16_t>::value) {
            EncTailP q{};
            if (with_x0) { q.pos = pos32; q.xf = xf[0]; q.xt = xt[0]; q.z0 = y2[0]; q.z1 = y2[1]; q.S = S; q.drop_p = dp; q.seed = site_seed(0); x0_done = true; }
            for (int k = 0; k < 2; ++k) {
                const EncW& e = encw(k); EncA& a = enca(k);
                EncTailCam& c = q.cam[k];
                c.x = e.gripper ? a.g0 : a.ss; c.W1 = e.fc1.W; c.W2 = e.fc2.W; c.b1 = e.fc1.b32; c.b2 = e.fc2.b32;
                c.lng = e.lng; c.lnb = e.lnb; c.f1 = a.f1; c.f2 = a.f2; c.lnst = a.lnst; c.col0 = k * 64;
            }
            q.emb = enc_emb(); q.Nf = Nf; q.ldemb = EMB;
            launch_enc_tail_fwd(st, q);
        }
    }
    // ---- weight-gradient slabs.  16-bit engines: the slab -> gradient reductions of the encoders' backward are collected and run as ONE launch (flush_unpacks)
    // after both encoders' backward instead of one ~6-20 us launch behind each weight-gradient kernel.  The slabs of the queued jobs lie back to back in `part`;
    // part + part_cur is where the next launch writes its slabs.
    UnpackBatch unpack_jobs{};
    int64_t part_cur = 0;
    int unpack_blocks = 0;
    bool unpack_room(int jobs, int64_t floats) const { return unpack_jobs.n + jobs <= UNPACK_MAX_JOBS && part_cur + floats <= this->partcap; }
    // queue the reduction of the nsplit slabs [O][I KH KW] at part + part_cur into grad (shape and nhwc as unpack_conv_wgrad_kernel takes them; ysplit: UnpackJob).
    // Returns the slabs' address and moves part_cur past them, or nullptr when the queue or the slab area is full (nothing changes)
    float* queue_unpack(float* grad, int O, int I, int KH, int KW, int nhwc, int nsplit, int ysplit) {
        const long long slab = (long long)O * I * KH * KW;
        if (!unpack_room(1, nsplit * slab)) return nullptr;
        float* const slabs = this->part + part_cur;
        UnpackJob& U = unpack_jobs.j[unpack_jobs.n++];
        U.part = slabs; U.grad = grad; U.slab = slab; U.nsplit = nsplit; U.O = O; U.I = I; U.KH = KH; U.KW = KW; U.nhwc = nhwc; U.blk0 = unpack_blocks; U.ysplit = ysplit;
        unpack_blocks += cdiv((int)slab, 1024); part_cur += nsplit * slab;
        return slabs;
    }
    void flush_unpacks() {
        constexpr int yparts = 8;      // same-box: 4 / 8 / 16 / 32 parts = 60 / 55 / 59 / 86 us (with 8 slab quads in flight per thread)
        // a job with ysplit == 0 spreads its slabs over the grid.y parts, each landing with one atomic per element; reproducible mode: one part, slabs in order
        if (repro) for (int i = 0; i < unpack_jobs.n; ++i) unpack_jobs.j[i].ysplit = 1;
        else for (int i = 0; i < unpack_jobs.n; ++i) if (unpack_jobs.j[i].ysplit == 0 && unpack_jobs.j[i].nsplit > 1) nd(ND_CONV_UNPACK_SPLIT);
        if (unpack_jobs.n > 0) hipLaunchKernelGGL(unpack_conv_wgrad_batched_kernel, dim3(unpack_blocks, repro ? 1 : yparts), dim3(256), 0, st, unpack_jobs);
        unpack_jobs.n = 0; part_cur = 0; unpack_blocks = 0;
    }
    // the data-gradient chain of both tails (LayerNorm, fc2, fc1) in one launch, then the weight / bias gradients of their Linear layers in one more
    bool tail_fc7_done = false;
    void enc_tail_bwd_both(int Nf) {
        if constexpr (std::is_same<T, h16_t>::value) {
            EncTailBwdP q{};
            for (int k = 0; k < 2; ++k) {
                const EncW& e = encw(k); EncA& a = enca(k);
                EncTailBwdCam& c = q.cam[k];
                c.f2 = a.f2; c.lnst = a.lnst; c.lng = e.lng; c.f1 = a.f1; c.W2t = e.fc2.Wt; c.W1t = e.fc1.Wt;
                c.xmask = a.g0; c.dlng = e.dlng; c.dlnb = e.dlnb;       // g0 is fc7's ReLU output; the static camera's tail input (ss) has no mask
                c.d_f2 = a.d_f2t; c.d_f1 = a.d_f1; c.dx_f32 = a.d_ss; c.dx_t = a.d_g0; c.col0 = k * 64;
            }
            q.demb = enc_demb(); q.Nf = Nf; q.ldemb = EMB;
            const int nblk = cdiv(Nf, 16);
            const bool slab_pg = repro && nblk > 1;      // reproducible mode: LayerNorm parameter partials stored per workgroup (cspart), summed in block order
            if (slab_pg) for (int k = 0; k < 2; ++k) q.cam[k].pg_slab = cspart + (long long)k * 2 * nblk * 64;
            if (!repro && Nf > 16) nd(ND_ENC_TAIL_LN);
            launch_enc_tail_bwd(st, q);
            if (slab_pg)
                for (int k = 0; k < 2; ++k) {
                    hipLaunchKernelGGL(colsum_final_kernel, dim3(1), dim3(256), 0, st, (const float*)q.cam[k].pg_slab, nblk, 64, encw(k).dlng, (float*)nullptr, 1.f);
                    hipLaunchKernelGGL(colsum_final_kernel, dim3(1), dim3(256), 0, st, (const float*)q.cam[k].pg_slab + (long long)nblk * 64, nblk, 64, encw(k).dlnb, (float*)nullptr, 1.f);
                }
            // weight / bias gradients of the four Linear layers (+ fc7): one launch of the streaming body (lin_bwd_stream_kernel), operands read as they lie, the frames
            // walked in one or two ranges (74 tiles at the model's shape: two).  Every range writes its own slab; the slabs are summed into the gradient by the encoders'
            // one unpack launch (no per-element atomics here: 1.5 M of them made this launch 39 us).  A job without room for its slabs (null) adds to the gradient itself, with fp32 atomics when there are two ranges
            const int nz = enc_tail_nsplit(Nf);
            if (!repro && nz > 1) nd(ND_LIN_BWD_ROWS);      // the five jobs' bias gradients: one atomic per column and row range
            LinStreamBatch bt{};
            int blk = 0;
            const bool cs_bias = repro && nz > 1;      // reproducible mode: the bias gradients are two-stage column sums behind the launch, not the row ranges' atomics
            auto add = [&](const T* dY, const T* X, const LinW& L, float* dW, float* slabs) {
                lin_stream_add(bt, blk, (const h16_t*)dY, (const h16_t*)X, L.K, Nf, L.N, L.K, dW, L.K, cs_bias ? nullptr : L.db, slabs, nz, 0);
            };
            for (int k = 0; k < 2; ++k) {
                const EncW& e = encw(k); EncA& a = enca(k);
                add(a.d_f2t, a.f1, e.fc2, e.fc2.dW, queue_unpack(e.fc2.dW, e.fc2.N, e.fc2.K, 1, 1, 0, nz, 1));
                add(a.d_f1, e.gripper ? a.g0 : a.ss, e.fc1, e.fc1.dW, queue_unpack(e.fc1.dW, e.fc1.N, e.fc1.K, 1, 1, 0, nz, 1));
            }
            // + the gripper camera's first Linear (3136 -> 128, dY = d_g0 which the launch above just wrote): its slabs are in the packed (NHWC)
            // column order of a3 and the unpack launch lands them in the torch layout (the conv weights' permutation with a 7 x 7 "kernel")
            const LinW& L = encG.fc7;
            float* const slabs7 = L.N == 128 && L.K == 3136 ? queue_unpack(L.dW, 128, 64, 7, 7, 1, nz, 1) : nullptr;
            tail_fc7_done = slabs7 != nullptr;      // else head_bwd runs fc7's weight gradient
            if (slabs7) add(aG.d_g0, aG.a3, L, nullptr, slabs7);
            launch_lin_stream(st, bt, blk);
            if (cs_bias) {
                for (int k = 0; k < 2; ++k) {
                    const EncW& e = encw(k); EncA& a = enca(k);
                    colsum(a.d_f2t, e.fc2.N, Nf, e.fc2.N, e.fc2.db);
                    colsum(a.d_f1, e.fc1.N, Nf, e.fc1.N, e.fc1.db);
                }
                if (slabs7) colsum(aG.d_g0, L.N, Nf, L.N, L.db);
            }
        }
    }
    // row ranges of the tails' weight-gradient launch (74 tiles: two ranges from 257 frames up)
    static int enc_tail_nsplit(int Nf) { return lin_stream_nsplit(2 * (1 * 4 + 8 * 1) + 2 * 25, Nf); }
    // reproducible mode runs the fused tail backward only when every job of its weight-gradient launch gets slabs (a job without slabs adds with atomics)
    bool enc_tail_bwd_room(int Nf) const {
        const int64_t nz = enc_tail_nsplit(Nf);
        return unpack_room(5, nz * (2 * (64ll * 512 + 512ll * 128) + 128ll * 3136));
    }
    h16_t* zero_page = nullptr;
    const h16_t* wgrad_zero_page() {
        if constexpr (std::is_same<T, h16_t>::value) { if (!zero_page) zero_page = alloc<h16_t>(128); }     // zero-initialised by alloc()
        return zero_page;
    }
    // implicit-GEMM weight gradient (the fp32 engine's form, the 16-bit engines' last resort): split-K slabs at part + part_cur; returns their number
    template <int TM, typename LB> int wgrad_gemm(const ConvW& c, const T* dy, const LB& lb, long long npix) {
        const int Kc = c.I * c.KH * c.KW;
        int nsplit = (int)std::min<long long>(std::max<long long>(1, npix / 2048), (this->partcap - part_cur) / ((long long)c.O * Kc));
        nsplit = std::min(nsplit, 256);
        EpiP ep = epi(this->part + part_cur, true); ep.z_stride = (long long)c.O * Kc;
        PixMajorLoaderT<T> la{}; la.p = dy; la.rows = c.O; la.ld = c.O;
        launch_gemm<T, TM, 64>(st, la, lb, dense_out(Kc), ep, c.O, Kc, (int)npix, 1, nsplit);
        return nsplit;
    }
    // The slab hand-off and the bias gradient behind every weight-gradient launch.  nsplit slabs at part + part_cur -> the layer's gradient: a joint (two-camera) launch
    // always queues them for the batched unpack (its room was checked first; the gripper job has fewer than 64), a single launch queues 64 slabs or more of a 16-bit
    // engine, the rest is one launch here.  tr: a raw-tile kernel ran — outside reproducible mode it added the bias gradient itself (atomics); else the column sum of dy
    void wgrad_finish(const ConvW& c, const T* dy, long long npix, int nsplit, bool tr, bool joint) {
        const bool many = std::is_same<T, h16_t>::value && nsplit >= 64;
        const int yparts = many && !repro ? 16 : 1;
        // slab parts over grid.y, each landing with one fp32 atomic per element.  16 parts: more (21 / 24 / 64 for conv3 / conv2 / conv1) made
        // every launch slower (23 / 11.3 / 10.9 us against 18.6 / 9.5 / 9.6: the scattered atomics, not the slab stream, are the cost)
        if (!((joint || many) && queue_unpack(c.dW, c.O, c.I, c.KH, c.KW, c.nhwc, nsplit, 0))) {
            if (yparts > 1) nd(ND_CONV_UNPACK_SPLIT);
            hipLaunchKernelGGL(unpack_conv_wgrad_kernel, dim3(cdiv(c.O * c.I * c.KH * c.KW, 1024), yparts), dim3(256), 0, st, this->part + part_cur, nsplit,   // fp32 (parity) mode: one deterministic pass, no atomics
                               (long long)c.O * c.I * c.KH * c.KW, c.dW, c.O, c.I, c.KH, c.KW, c.nhwc);
        }
        if (!tr || repro) colsum(dy, c.O, (int)npix, c.O, c.db);      // reproducible mode: no bias atomics, the two-stage column sum
        else if (nsplit > 1) nd(ND_CONV_BIAS);
    }
    // conv3's / conv2's raw-tile + transposing-LDS-read launch (conv_wgrad.h; 16-bit engines) of camera s alone, or of s and g — both cameras — as ONE launch
    // (launch_conv_wgrad_pair).  ns = slabs (= persistent workgroups) per camera; false = nothing launched (the fp32 engine, a shape the launchers do not take, no room)
    bool conv_wgrad_launch(const Stage& s, const Stage* g, int* ns) {
        if constexpr (std::is_same<T, h16_t>::value) {
            const ConvW& c = s.c;
            const bool is3 = c.I == 64 && c.KH == 3, is2 = c.I == 32 && c.KH == 4;
            if (!is3 && !is2) return false;
            if (g && (g->c.I != c.I || g->c.KH != c.KH || g->c.O != c.O || c.O != 64 || !unpack_room(2, 256 * (int64_t)c.O * c.I * c.KH * c.KW))) return false;
            // reproducible mode: strided items (no claim counter) and no bias atomics
            auto job = [&](const Stage& q) {
                WgradJob J{}; J.X = q.x; J.dY = q.dy; J.part = this->part + part_cur; J.bias_part = repro ? nullptr : q.c.db; J.zeros = wgrad_zero_page(); J.Nf = q.g.Nf; J.IH = q.g.IH; J.IW = q.g.IW; J.OH = q.g.OH; J.OW = q.g.OW; J.work_ctr = claim_ctr(q.g.Nf > 1); J.FPB = 1;
                return J;
            };
            const WgradJob A = job(s), B = g ? job(*g) : WgradJob{};
            TimerScope ts(this, "conv_wgrad_tr", "mfma", 0, 0, 0);
            bool ok;
            if (g) ok = is3 ? launch_conv_wgrad_pair<64, 64, 3, 3, 1>(st, A, B, 512, nullptr, ns) : launch_conv_wgrad_pair<32, 64, 4, 4, 2>(st, A, B, 512, nullptr, ns);
            else ok = (ns[0] = is3 ? launch_conv_wgrad_tr<64, 64, 3, 3, 1>(st, A, 512) : launch_conv_wgrad_tr<32, 64, 4, 4, 2>(st, A, 512)) > 0;
            if (ok) ts.add(conv_wgrad_flops(c, s.g) + (g ? conv_wgrad_flops(g->c, g->g) : 0), conv_wgrad_bytes(c, s.g, 2) + (g ? conv_wgrad_bytes(g->c, g->g, 2) : 0));
            return ok;
        }
        return false;
    }
    // conv3's / conv2's weight gradient of cameras [k0, k1): the joint launch when the range holds both cameras, else per camera the single launch, or the implicit
    // GEMM (the fp32 engine's form, the 16-bit engines' last resort)
    void conv_wgrad(int k0, int k1, int sn, int Nf) {
        auto npix = [](const Stage& s) { return (long long)s.g.Nf * s.g.OH * s.g.OW; };
        if (k1 - k0 == 2) {
            const Stage S = stage(k0, sn, Nf), G = stage(k0 + 1, sn, Nf);
            int ns[2] = {0, 0};
            if (conv_wgrad_launch(S, &G, ns)) {
                wgrad_finish(S.c, S.dy, npix(S), ns[0], true, true);
                wgrad_finish(G.c, G.dy, npix(G), ns[1], true, true);
                return;
            }
        }
        for (int k = k0; k < k1; ++k) {
            const Stage s = stage(k, sn, Nf);
            int nsplit = 0;
            const bool tr = conv_wgrad_launch(s, nullptr, &nsplit);
            if (!tr) nsplit = wgrad_gemm<64>(s.c, s.dy, ConvNHWCLoaderT<T>{s.x, s.g}, npix(s));
            wgrad_finish(s.c, s.dy, npix(s), nsplit, tr, false);
        }
    }
    // conv1's launch (conv1_wgrad.h launch_conv1_wgrad_jobs; 16-bit engines) of the jobs [cameras ka, kb) x [frame sources ha, hb) in that order, so a camera's slabs lie
    // together.  Paired pass: two sources per camera, as conv1_fwd.  ns = slabs per job; false = nothing launched (the fp32 engine, or the jobs take different kernel forms)
    bool conv1_wgrad_launch(int ka, int kb, int ha, int hb, const Conv1Src* src, const Conv1Src* src2, int Nf, int* ns) {
        if constexpr (std::is_same<T, h16_t>::value) {
            Wgrad1Job J[4]; int nj = 0;
            double fl = 0, by = 0;
            for (int k = ka; k < kb; ++k) {
                for (int h = ha; h < hb; ++h) {
                    const int nf = src2 ? src_frames(Nf, h) : Nf;
                    const ConvGeom g = geom(nf, encw(k).IH, 3, 8, 4);
                    Wgrad1Job q{}; q.S = h ? src2[k] : src[k]; q.work_ctr = claim_ctr(nf > 1); q.dY = enca(k).dact1 + (long long)(h ? src_frames(Nf, 0) : 0) * g.OH * g.OW * 32; q.bias_part = repro ? nullptr : encw(k).c1.db;
                    q.Nf = nf; q.IH = g.IH; q.IW = g.IW; q.OH = g.OH; q.OW = g.OW;
                    J[nj++] = q;
                    fl += conv_wgrad_flops(encw(k).c1, g); by += conv_wgrad_bytes(encw(k).c1, g, q.S.u8 ? 1 : 4);
                }
            }
            J[0].part = this->part + part_cur;
            TimerScope ts(this, "conv1_wgrad", "hbm", 0, 0, 0);
            if (!launch_conv1_wgrad_jobs(st, J, nj, 1024, nullptr, ns)) return false;
            ts.add(fl, by);
            return true;
        }
        return false;
    }
    // conv1's weight gradient of cameras [k0, k1): both cameras (and both frame sources of each) as one launch when the range holds both, else once per camera and
    // frame source.  The fp32 engine reads the frames the forward materialised (conv1_f32)
    void conv1_wgrad(int k0, int k1, const Conv1Src* src, const Conv1Src* src2, int Nf) {
        const int ns_src = src2 ? 2 : 1;
        if (k1 - k0 == 2) {
            const ConvW &cS = encw(k0).c1, &cG = encw(k0 + 1).c1;
            int ns[4] = {0, 0, 0, 0};
            if (cS.O == 32 && cG.O == 32 && cS.I * cS.KH * cS.KW == 192 && cG.I * cG.KH * cG.KW == 192 && unpack_room(2, 1024 * (int64_t)32 * 192) &&      // (at most max_blocks = 1024 slabs)
                conv1_wgrad_launch(k0, k1, 0, ns_src, src, src2, Nf, ns)) {
                for (int k = k0; k < k1; ++k) {      // a camera's slabs are one job of the batched unpack; its bias gradient runs over all its frames (both sources' rows of dact1 lie back to back)
                    const ConvGeom g = geom(Nf, encw(k).IH, 3, 8, 4);
                    wgrad_finish(encw(k).c1, enca(k).dact1, (long long)Nf * g.OH * g.OW, ns[(k - k0) * ns_src] + (src2 ? ns[(k - k0) * ns_src + 1] : 0), true, true);
                }
                return;
            }
        }
        for (int k = k0; k < k1; ++k) {
            const EncW& e = encw(k);
            for (int h = 0; h < ns_src; ++h) {
                const int nf = src2 ? src_frames(Nf, h) : Nf;
                const ConvGeom g = geom(nf, e.IH, 3, 8, 4);
                const long long npix = (long long)nf * g.OH * g.OW, foff = h ? src_frames(Nf, 0) : 0;
                const T* dy = enca(k).dact1 + foff * g.OH * g.OW * 32;
                int nsplit = 0;
                const bool tr = conv1_wgrad_launch(k, k + 1, h, h + 1, src, src2, Nf, &nsplit) && nsplit > 0;
                if (!tr) {
                    const Conv1Src& sh = h ? src2[k] : src[k];
                    const float* x = nullptr;
                    if constexpr (std::is_same<T, float>::value) x = sh.u8 ? x32[k] + foff * 3 * e.IH * e.IH : reinterpret_cast<const float*>(sh.X);
                    nsplit = wgrad_gemm<32>(e.c1, dy, Conv1LoaderT<T>{x, g}, npix);
                }
                wgrad_finish(e.c1, dy, npix, nsplit, tr, false);
            }
        }
    }
    ConvTileP conv_dgrad_job(const Stage& s, bool bits) {
        ConvTileP p{};
        if constexpr (std::is_same<T, h16_t>::value) {
            p.img = s.dy; p.IMH = s.g.OH; p.IMW = s.g.OW; p.w = s.c.Wd; p.out = s.dx; p.OUTH = s.g.IH; p.OUTW = s.g.IW; p.mask = bits ? nullptr : s.x; p.maskbits = bits ? s.xbits : nullptr; p.Nf = s.g.Nf; p.work_ctr = next_ctr();
            if (!zero_page) zero_page = alloc<h16_t>(128);      // zero-initialised by alloc(): the staged zero border of the data-gradient form
            p.zeros = zero_page;
            if (!dump_page) dump_page = alloc<h16_t>(4096);
            p.dump = dump_page;
        }
        return p;
    }
    // algorithmic bytes as SURVEY 8(d) counts them: dY read once, dX written once, 2 B each; the ReLU mask of the layer below is read as BIT words
    // (pin * I / 8 bytes) when the forward left them, as a second 16-bit activation read otherwise (VERDICT r5 weak #4: the bit form was priced as a full read)
    static double conv_dgrad_flops(const ConvW& c, const ConvGeom& g) { return 2.0 * g.Nf * g.OH * g.OW * c.O * c.I * c.KH * c.KW; }
    static double conv_dgrad_bytes(const ConvW& c, const ConvGeom& g, bool bits, bool mask) {
        const double pin = (double)g.Nf * g.IH * g.IW, pout = (double)g.Nf * g.OH * g.OW;
        return (pout * c.O + pin * c.I) * 2 + (bits ? pin * c.I / 8 : (mask ? pin * c.I * 2 : 0));
    }
    static bool dgrad_is3(const ConvW& c) { return c.KH == 3 && c.S == 1 && c.I == 64 && c.O == 64; }
    static bool dgrad_is2(const ConvW& c) { return c.KH == 4 && c.S == 2 && c.I == 32 && c.O == 64; }
    // the data gradient of one stage (conv3 or conv2) for BOTH cameras as one launch: the production bitmask form, both jobs on the same instantiation.
    // false = nothing launched (a shape / mask form the merged launch does not take)
    bool conv_dgrad_both(int sn, int Nf) {
        if constexpr (std::is_same<T, h16_t>::value) {
            const Stage S = stage(0, sn, Nf), G = stage(1, sn, Nf);
            if (!S.xbits || !G.xbits) return false;
            const bool k3 = dgrad_is3(S.c) && dgrad_is3(G.c), k2 = dgrad_is2(S.c) && dgrad_is2(G.c);
            if (!k3 && !k2) return false;
            const ConvTileP j[2] = {conv_dgrad_job(S, true), conv_dgrad_job(G, true)};
            TimerScope ts(this, "conv_tile_dgrad", "mfma", 0, 0, 0);
            const bool ok = k3 ? launch_conv_reg_jobs<64, 3, 3, 1, true, 1, 4, true, 1>(st, j, 2) : launch_conv_reg_jobs<64, 2, 2, 1, true, 2, 4, true, 1>(st, j, 2);
            if (ok) ts.add(conv_dgrad_flops(S.c, S.g) + conv_dgrad_flops(G.c, G.g), conv_dgrad_bytes(S.c, S.g, true, false) + conv_dgrad_bytes(G.c, G.g, true, false));
            return ok;
        }
        return false;
    }
    // the data gradient of conv3 / conv2 of one camera, masked by the ReLU of the layer below
    void conv_dgrad(int k, int sn, int Nf) {
        const Stage s = stage(k, sn, Nf);
        const ConvW& c = s.c; const ConvGeom& g = s.g;
        if constexpr (std::is_same<T, h16_t>::value) {
            const bool bits = s.xbits != nullptr;
            ConvTileP p = conv_dgrad_job(s, bits);
            bool ok = false;
            TimerScope ts(this, "conv_tile_dgrad", "mfma", conv_dgrad_flops(c, g), conv_dgrad_bytes(c, g, bits, true));
            // both data gradients run on conv_reg.h's pipelined-epilogue form (EPI: a tile's epilogue rides in the next tile's multiply loop), two 256-thread workgroups per CU
            if (dgrad_is3(c)) ok = (bits && launch_conv_reg<64, 3, 3, 1, true, 1, 4, true, 1>(st, p)) || launch_conv_tile<64, 64, 3, 3, 1, 1, true>(st, p);
            else if (dgrad_is2(c)) ok = (bits && launch_conv_reg<64, 2, 2, 1, true, 2, 4, true, 1>(st, p)) || launch_conv_tile<64, 32, 2, 2, 1, 2, true>(st, p);
            if (ok) return;
        }
        ConvDgradLoader<T> l{s.dy, g, c.O};
        DgradOut om{g};
        EpiP ep = epi(s.dx, false); ep.mask = s.x;
        const int ncls = g.S * g.S;
        const int Kd = (g.KH / g.S) * (g.KW / g.S) * c.O;
        const int Ic = (g.IH + g.S - 1) / g.S;
        const int Mmax = g.Nf * Ic * Ic;
        for (int zc = 0; zc < ncls; ++zc)   // one launch per parity class: the packed weight slab differs per class
            launch_dgrad(l, dense<T>(c.Wd + (long long)zc * c.I * Kd, c.I, Kd), om, ep, Mmax, c.I, Kd, zc);
    }
    void launch_dgrad(const ConvDgradLoader<T>& l, const DenseLoader<T>& wb, const DgradOut& om, const EpiP& ep, int Mmax, int N, int K, int zc) {
        // one parity class per launch: wrap the loader/out-map so that blockIdx.z == 0 maps to class zc
        ClassShift<ConvDgradLoader<T>> ls{l, zc};
        ClassShiftOut<DgradOut> os{om, zc};
        if (N <= 32) launch_gemm<T, 128, 32>(st, ls, wb, os, ep, Mmax, N, K);
        else launch_gemm<T, 128, 64>(st, ls, wb, os, ep, Mmax, N, K);
    }
    template <typename L> struct ClassShift {
        static constexpr bool TRANSPOSED = false;
        L l; int zc;
        using Row = typename L::Row;
        DEVI int num_rows(int) const { return l.num_rows(zc); }
        DEVI Row row(int r, int) const { return l.row(r, zc); }
        DEVI void fetch(const Row& c, int k0, int kend, T (&v)[8]) const { l.fetch(c, k0, kend, v); }
    };
    template <typename O> struct ClassShiftOut {
        O o; int zc;
        DEVI long long offset(int r, int) const { return o.offset(r, zc); }
    };
    // one camera's backward from the gradient of its embedding columns down to the gradient of a3.  tail_done: enc_tail_bwd_both has run the tail (LayerNorm, fc2, fc1)
    // with its weight gradients, and fc7's weight gradient too if tail_fc7_done
    void head_bwd(int k, int Nf, bool tail_done) {
        const EncW& e = encw(k); EncA& a = enca(k);
        if (!tail_done) {
            ln_bwd(enc_demb() + k * 64, EMB, a.f2, 64, a.lnst, e.lng, Nf, 64, nullptr, 0, 0, a.d_f2t, 64, e.dlng, e.dlnb);
            { EpiP ep = epi(a.d_f1, false); ep.mask = a.f1; lin_dgrad(a.d_f2t, Nf, e.fc2, ep, dense_out(512)); }
            lin_wgrad(a.d_f2t, a.f1, 512, Nf, 64, 512, e.fc2.dW, 512, e.fc2.db);
        }
        if (!e.gripper) {
            if (!tail_done) {
                { EpiP ep = epi(a.d_ss, true); lin_dgrad(a.d_f1, Nf, e.fc1, ep, dense_out(128)); }
                lin_wgrad(a.d_f1, a.ss, 128, Nf, 512, 128, e.fc1.dW, 128, e.fc1.db);
            }
            if constexpr (std::is_same<T, h16_t>::value) launch_spatial_softmax64_bwd(st, a.a3, a.ssstats, a.d_ss, Nf, e.H3, e.H3, a.dact3);
            else hipLaunchKernelGGL((spatial_softmax_bwd_kernel<T>), dim3(Nf), dim3(256), 0, st, a.a3, a.ssstats, a.d_ss, e.H3, e.H3, 64, a.dact3);
        } else {
            if (!tail_done) {
                { EpiP ep = epi(a.d_g0, false); ep.mask = a.g0; lin_dgrad(a.d_f1, Nf, e.fc1, ep, dense_out(128)); }
                lin_wgrad(a.d_f1, a.g0, 128, Nf, 512, 128, e.fc1.dW, 128, e.fc1.db);
            }
            { EpiP ep = epi(a.dact3, false); ep.mask = a.a3; lin_dgrad(a.d_g0, Nf, e.fc7, ep, dense_out(3136)); }
            // dW7 in packed (NHWC) column order -> temp, then permute-accumulate into the torch-layout grad
            if (!(tail_done && tail_fc7_done)) {
                lin_wgrad(a.d_g0, a.a3, 3136, Nf, 128, 3136, dw7_tmp, 3136, e.fc7.db);
                hipLaunchKernelGGL((permute_cols_kernel<float, float>), dim3(cdiv(128 * 3136, 256)), dim3(256), 0, st, dw7_tmp, e.fc7.dW, 128, 64, 49, 1, 1);
            }
        }
    }
    // The encoders' backward of cameras [k0, k1): the stage list of enc_fwd_stages in reverse — per camera down to the gradient of a3, then the weight gradient and
    // the data gradient of conv3 and of conv2, then conv1's weight gradient, each as the two-camera launch or once per camera.  In the 16-bit engines each camera
    // has its own gradient buffers, since both cameras' gradients of a stage are alive at once.
    void enc_bwd_stages(int k0, int k1, const Conv1Src* src, const Conv1Src* src2, int Nf, bool tail_done) {
        const bool both = k1 - k0 == 2;
        for (int k = k0; k < k1; ++k) head_bwd(k, Nf, tail_done);
        for (int sn = 3; sn >= 2; --sn) {
            conv_wgrad(k0, k1, sn, Nf);
            if (!(both && conv_dgrad_both(sn, Nf))) for (int k = k0; k < k1; ++k) conv_dgrad(k, sn, Nf);
        }
        conv1_wgrad(k0, k1, src, src2, Nf);
    }
    void enc_bwd_both(const Conv1Src* src, const Conv1Src* src2, int Nf, bool tail_done) {
        if constexpr (std::is_same<T, h16_t>::value) enc_bwd_stages(0, 2, src, src2, Nf, tail_done);
        else for (int k = 0; k < 2; ++k) enc_bwd_stages(k, k + 1, src, src2, Nf, tail_done);
    }
