// THE on / off decision of a prediction logit and of a target value, shared by every unit that scores or draws a mask
// (data.hip: overlap counters, label maps, restored volumes; contour.hip: contour distances).
#pragma once
#include <hip/hip_runtime.h>

namespace glf {

__device__ __forceinline__ float sigmoid_d(float x) { return 1.0f / (1.0f + expf(-x)); }
// THE binarisation of a logit (main.py:250, 385, 606): metrics, label maps and restored volumes all decide a pixel here.
// Logit 0.0, -0.0, -inf and NaN are off, +inf is on.
__device__ __forceinline__ bool channel_on(float x) { return sigmoid_d(x) > 0.5f; }
// a target pixel counts as set when it is not zero (main.py:803-806 compare a 0/1 mask)
__device__ __forceinline__ bool target_on(float t) { return t != 0.f; }

}  // namespace glf
