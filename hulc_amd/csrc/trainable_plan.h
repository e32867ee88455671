// hulc_amd/csrc/trainable_plan.h — host-only arithmetic of the per-tensor trainable mask (engine_trainable.inc): the refusals of hulc_trainable_set /
// hulc_trainable_steps_set that need no device, the switch between a tensor's two counts and the grouping by sat-out count.  No HIP in here: the host tests
// compile it on its own (tests/test_trainable_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace hulc_trainable {

constexpr int MAX_GROUPS = 8;      // distinct sat-out counts alive among the trainable tensors (kernels.h OPT_GROUPS: the per-group numbers ride in the kernel arguments)

// 0 = the call may go on; else `err` holds the message
inline int check_call(const char* who, bool bound, long long n_bound, long long n, char* err, size_t cap) {
    if (!bound) { snprintf(err, cap, "%s before hulc_bind_params", who); return 1; }
    if (n != n_bound) { snprintf(err, cap, "%s: %lld entries, %lld tensors are bound", who, n, n_bound); return 1; }
    return 0;
}
// torch.optim keeps `step` per parameter.  Per tensor ONE count is kept: while it trains, the optimizer steps it sat out (constant); while it is frozen, the
// steps it has taken (constant).  `taken` optimizer steps have been taken when the mask changes: a tensor that switches converts one into the other
inline void apply_mask(const uint8_t* want, long long taken, std::vector<uint8_t>& mask, std::vector<int64_t>& cnt) {
    for (size_t t = 0; t < mask.size(); ++t) {
        const uint8_t w = want[t] ? 1 : 0;
        if (w != mask[t]) { cnt[t] = taken - cnt[t]; mask[t] = w; }
    }
}
// sat-out counts of all tensors, whatever their state
inline long long frozen_steps(uint8_t trainable, int64_t cnt, long long taken) { return trainable ? cnt : taken - cnt; }
// the distinct sat-out counts of the trainable tensors, ascending; 1 (and the message) when there are more than MAX_GROUPS
inline int plan_groups(const char* who, const std::vector<uint8_t>& mask, const std::vector<int64_t>& cnt, std::vector<int64_t>& offs, char* err, size_t cap) {
    offs.clear();
    for (size_t t = 0; t < mask.size(); ++t) if (mask[t] && std::find(offs.begin(), offs.end(), cnt[t]) == offs.end()) offs.push_back(cnt[t]);
    std::sort(offs.begin(), offs.end());
    if (offs.size() > (size_t)MAX_GROUPS) {
        snprintf(err, cap, "%s: the trainable tensors would hold %d distinct frozen-step counts, the limit is %d (freeze and unfreeze in fewer batches)", who, (int)offs.size(), MAX_GROUPS);
        return 1;
    }
    return 0;
}

}  // namespace hulc_trainable
