// What the forward of the two geometry terms of calc_loss_contact (csrc/corr_losses.hip) and their backward (csrc/corr_geometry_grad.hip) share: the tiling
// of a frame's queries, the exact squared distance, the posing of a canonical object point and the fixed-order workgroup sum.  Both passes must reach the
// same nearest neighbour from the same bits, so these exist once.
#pragma once
#include "common.h"

namespace idf_corr_geometry {

constexpr int CL_THR = 256, CL_QPT = 4, CL_TILE = CL_THR * CL_QPT;      // queries per workgroup
constexpr int CL_RC = 1024;                                            // reference points per LDS chunk
constexpr int HV = 7;                                                  // floats per body vertex record: position 3 | normal 3 | contact label

// squared distance with every operation rounded on its own (the contract of csrc/geometry.hip nn_argmin)
__device__ __forceinline__ float cl_dist2(float qx, float qy, float qz, float rx, float ry, float rz) {
#pragma clang fp contract(off)
    const float dx = qx - rx, dy = qy - ry, dz = qz - rz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// p' = M p + t with M = rotation_6d_to_matrix(pred) -- train_correction_smpl.py:121,126 multiplies the row vector by the transposed
// matrix.  Products and sums rounded one by one, left to right (what an elementwise restatement computes).
__device__ __forceinline__ float3 cl_pose(const float *R, float px, float py, float pz) {
#pragma clang fp contract(off)
    float3 o;
    o.x = ((R[0] * px + R[1] * py) + R[2] * pz) + R[9];
    o.y = ((R[3] * px + R[4] * py) + R[5] * pz) + R[10];
    o.z = ((R[6] * px + R[7] * py) + R[8] * pz) + R[11];
    return o;
}

// fixed-order sum of the workgroup's per-thread values: LDS tree, the same pairs whatever the data
__device__ __forceinline__ float cl_tree(float v, float *sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = CL_THR / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    return sm[0];
}

}  // namespace idf_corr_geometry
