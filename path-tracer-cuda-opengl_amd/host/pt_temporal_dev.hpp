// pt_temporal_dev.hpp — pt_film_temporal's reprojection pass on the device (csrc/pt_temporal.hip).
//
// Like the a-trous pass it is an image kernel with no tie to the traversal code, so it lives in a
// translation unit of its own; pt_film_temporal (pt_device.hip, where pt_film is defined) validates,
// owns the two history images and the previous camera, and enqueues one launch per call.
#pragma once
#include <hip/hip_runtime.h>

#include "pt.h"

namespace pt {

constexpr size_t kHistoryBytes = 48;   // a history pixel: three 16-byte rows {acc.rgb, len}{n, mat}{p, hit flag}

struct TemporalParams {
    float o[3], ll[3], hor[3], ver[3];   // the previous camera (read only when haveHistory)
    float maxHistory, sigmaPlane, normalCos;
    int width, height;
    int haveHistory;   // the film holds a history image of this size
    int linear;        // PT_TEMPORAL_LINEAR
};

// include/pt.h's rule: rgb, aov (the frame; each pixel reads them only at itself, so out may be rgb) and
// the old history `prev` (W x H x 3 float4 rows, gathered) -> out, outLen (may be NULL) and the new
// history `next`, which must not overlap `prev`.
hipError_t temporalPass(const float* rgb, const pt_aov* aov, const void* prev, void* next, float* out, float* outLen,
                        const TemporalParams& params, hipStream_t stream);

}  // namespace pt
