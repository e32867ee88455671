// hulc_amd/csrc/store_gather.h — hulc_store_gather (include/hulc_hip.h): the non-image half of a frame-store batch, assembled on the device from
// per-frame tables that live next to the store.  Same window arithmetic as the frames (window_rows.h window_expand_kernel): L = clamp(window_len[b], 1, S),
// s0 = clamp(window_start[b], 0, F - L), row (b, t) = table row s0 + min(t, L - 1).  Padding (t >= L) restates calvin_agent's _pad_sequence:
// robot_obs repeats the last real row; RELATIVE actions pad dims 0..5 with zeros and repeat dim 6 (the gripper); ABSOLUTE actions repeat all seven.
// Copies and zeros only: the result is exact.  Included by capi.hip alone.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hulc_hip.h"

struct StoreGatherP {
    const float *actions, *robot_obs, *lang;
    const long long* wstart;
    const int* wlen;
    const int* lang_row;
    float *act_out, *ro_out, *lang_out;
    long long F;
    int A, B, S, absolute;
};
__global__ void __launch_bounds__(256) store_gather_kernel(StoreGatherP p) {
    const int n_fr = p.B * p.S * 22, n_lang = p.lang_out ? p.B * 384 : 0;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n_fr) {
        const int row = idx / 22, c = idx - row * 22;             // columns 0..6: actions, 7..21: robot_obs
        const int b = row / p.S, t = row - b * p.S;
        const int L = p.wlen ? min(max(p.wlen[b], 1), (int)min((long long)p.S, p.F)) : (int)min((long long)p.S, p.F);
        const long long s0 = min(max(p.wstart[b], 0ll), p.F - (long long)L);
        const long long src = s0 + min(t, L - 1);
        if (c < 7) p.act_out[(long long)row * 7 + c] = (t >= L && !p.absolute && c < 6) ? 0.f : p.actions[src * 7 + c];
        else p.ro_out[(long long)row * 15 + (c - 7)] = p.robot_obs[src * 15 + (c - 7)];
    } else if (idx < n_fr + n_lang) {
        const int e = idx - n_fr, b = e / 384, k = e - b * 384;
        const int r = min(max(p.lang_row[b], 0), p.A - 1);
        p.lang_out[e] = p.lang[(long long)r * 384 + k];
    }
}
