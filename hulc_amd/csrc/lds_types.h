// hulc_amd/csrc/lds_types.h — what the raw-tile kernels share about LDS: 16-byte vector and 32-bit LDS pointer types, the transposing fragment read
// (ds_read_b64_tr_b16, semantics in conv_wgrad.h) and the float division by a loop-invariant divisor their slot decoders use.  Used by the conv weight gradients,
// conv1's staging, the Linear backward, the conv forward / data-gradient tiles, the encoder tails and the fused transformer layers.
#pragma once
#include "common.h"

namespace HULC_NS {

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4_t lds_u32x4;

typedef __attribute__((address_space(3))) char lds_char;      // 32-bit LDS pointers: half the address registers of generic ones
DEVI h16x8_t tr_read8(lds_char* p0, lds_char* p1) {
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p0);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p1);
    typedef short s16x8_t __attribute__((ext_vector_type(8)));
    const s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(h16x8_t, v);
}
DEVI int wg_fdiv(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }

}  // namespace HULC_NS
