// float3 helpers of the geometry kernels (geometry.hip, optimize.hip, contact_scan.h): one definition.  Plain expressions -- how a caller's
// products and sums are contracted is decided where they are inlined, by that kernel's own `fp contract` setting.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float3 ld3(const float *p) { return make_float3(p[0], p[1], p[2]); }
__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 cross3(float3 a, float3 b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

}  // namespace
