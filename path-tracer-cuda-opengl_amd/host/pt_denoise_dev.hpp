// pt_denoise_dev.hpp — one pass of pt_film_denoise's a-trous filter on the device (csrc/pt_denoise.hip).
//
// The filter is an image kernel with no tie to the traversal code, so it lives in a translation unit
// of its own; pt_film_denoise (pt_device.hip, where pt_film is defined) validates, owns the scratch
// images and enqueues one pass per iteration.
#pragma once
#include <hip/hip_runtime.h>

#include "pt.h"

namespace pt {

// Pass with tap spacing `step` (1 << i) of include/pt.h's rule: in -> out, both W x H x 3 floats (they
// must not overlap), aov W x H records; isa2, isc2 = the pass's constants as pt.h defines them.
hipError_t atrousPass(const float* in, const pt_aov* aov, float* out, int width, int height, int step, float isa2,
                      float isc2, float sigmaPlane, hipStream_t stream);

}  // namespace pt
