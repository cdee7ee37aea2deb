// luma_level.h -- THE luma level of a pixel: the one definition niqe.hip (resr_niqe_luma_*) and fullref.hip (resr_fullref) share.
//   t = r * 65.481f; t += g * 128.553f; t += b * 24.966f; t += 16.0f; level = rint(t) -- six fp32 operations, each rounded once, in
//   this order (contraction off); a byte enters as unit_of_byte: (float)byte / 255.0f.  tests/niqe_ref.niqe_luma_np states the same
//   chain in numpy and is the definition.
#pragma once
#include "common.h"

namespace resr {

// (the pragma, not __fmul_rn / __fadd_rn: those are plain operators in this toolchain, and the build's default contraction turned
// them into fused multiply-adds -- 37 of the 2^24 byte triples then rounded the other way)
__device__ __forceinline__ uint8_t niqe_level(float r, float g, float b) {
#pragma clang fp contract(off)
    float t = r * 65.481f;
    t = t + g * 128.553f;
    t = t + b * 24.966f;
    t = t + 16.0f;
    t = rintf(t);                                   // half to even, as torch.round
    return (uint8_t)fminf(fmaxf(t, 0.f), 255.f);    // 16..235 for inputs in [0, 1]; anything else is pinned into a byte
}

// a byte of a uint8 frame as the network's unit value: the correctly rounded division of the build's default, as yuv.h's unit_of (all
// 2^24 triples are tested)
__device__ __forceinline__ float unit_of_byte(uint8_t v) { return (float)v / 255.0f; }

}  // namespace resr
