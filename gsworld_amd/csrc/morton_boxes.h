// morton_boxes.h -- the pieces of a Morton-ordered box search that knn.hip (distCUDA2: one cloud against itself) and
// nnquery.hip (nearest point of a second cloud) share: bounds of a cloud, 30-bit Morton codes in those bounds, the gather
// of the sorted points with the AABBs of boxes of kBox consecutive ones, the one squared-distance chain, and the lane
// broadcast of the streaming loop.  Kernels live in an unnamed namespace: each translation unit gets its own copy.
#pragma once

#include <float.h>

#include "gsr_internal.h"

namespace {

constexpr int kBox = 1024;

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

__global__ __launch_bounds__(GSR_BLOCK) void knn_minmax_partial_kernel(int P, const float *__restrict__ pts,
                                                                       float *__restrict__ partial) {
    __shared__ float s_red[4][6];
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * GSR_BLOCK + (int)threadIdx.x; i < P; i += gridDim.x * GSR_BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = pts[3 * (size_t)i + c];
            mn[c] = fminf(mn[c], v);
            mx[c] = fmaxf(mx[c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
    if (gsr_lane() == 0)
        for (int c = 0; c < 3; c++) {
            s_red[gsr_wave()][c] = mn[c];
            s_red[gsr_wave()][3 + c] = mx[c];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = (int)threadIdx.x;
        float v = s_red[0][c];
        for (int w = 1; w < 4; w++) v = c < 3 ? fminf(v, s_red[w][c]) : fmaxf(v, s_red[w][c]);
        partial[blockIdx.x * 6 + c] = v;
    }
}

__global__ void knn_minmax_final_kernel(int nblocks, const float *__restrict__ partial, float *__restrict__ minmax,
                                        uint32_t *n_dev, uint32_t P) {
    const int c = (int)threadIdx.x;
    if (c < 6) {
        float v = partial[c];
        for (int b = 1; b < nblocks; b++) v = c < 3 ? fminf(v, partial[b * 6 + c]) : fmaxf(v, partial[b * 6 + c]);
        minmax[c] = v;
    }
    if (c == 0) *n_dev = P;
}

// 10 bits per axis, x in the lowest interleave position
__device__ __forceinline__ uint32_t spread10(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// code of a point in the grid of `minmax` (min xyz, max xyz); a point outside is clamped to the grid's faces
__device__ __forceinline__ uint32_t morton_code(const float (&v)[3], const float *__restrict__ minmax) {
    uint32_t code = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float lo = minmax[c], hi = minmax[3 + c];
        const float ext = hi - lo;
        float t = ext > 0.f ? (v[c] - lo) / ext : 0.f;
        t = fminf(fmaxf(t, 0.f), 1.f);
        code |= spread10((uint32_t)(t * 1023.0f)) << c;
    }
    return code;
}

__global__ __launch_bounds__(GSR_BLOCK) void knn_morton_kernel(int P, const float *__restrict__ pts,
                                                               const float *__restrict__ minmax,
                                                               uint32_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int i = blockIdx.x * GSR_BLOCK + (int)threadIdx.x;
    if (i >= P) return;
    const float v[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    keys[i] = morton_code(v, minmax);
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(GSR_BLOCK) void knn_gather_box_kernel(int P, const float *__restrict__ pts,
                                                                   const uint32_t *__restrict__ order,
                                                                   float *__restrict__ sorted_pts,
                                                                   float *__restrict__ boxes) {
    // one workgroup per box of 1024 sorted points: gather them and reduce their AABB
    __shared__ float s_red[4][6];
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int k = 0; k < kBox / GSR_BLOCK; k++) {
        const int s = blockIdx.x * kBox + k * GSR_BLOCK + (int)threadIdx.x;
        if (s < P) {
            const uint32_t g = order[s];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float v = pts[3 * (size_t)g + c];
                sorted_pts[3 * (size_t)s + c] = v;
                mn[c] = fminf(mn[c], v);
                mx[c] = fmaxf(mx[c], v);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
    if (gsr_lane() == 0)
        for (int c = 0; c < 3; c++) {
            s_red[gsr_wave()][c] = mn[c];
            s_red[gsr_wave()][3 + c] = mx[c];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = (int)threadIdx.x;
        float v = s_red[0][c];
        for (int w = 1; w < 4; w++) v = c < 3 ? fminf(v, s_red[w][c]) : fmaxf(v, s_red[w][c]);
        boxes[blockIdx.x * 6 + c] = v;
    }
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fma_(dz, dz, fma_(dy, dy, dx * dx));
}

// Lower bound of dist2(p, any point of the box b = min xyz, max xyz) with the same fmaf chain: each |component| is <= the
// true one, and the chain is monotone in them, so the bound never exceeds the distance to a point inside.
__device__ __forceinline__ float box_dist2(float px, float py, float pz, const float *__restrict__ bx) {
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (px < bx[0] || px > bx[3]) dx = fminf(fabsf(px - bx[0]), fabsf(px - bx[3]));
    if (py < bx[1] || py > bx[4]) dy = fminf(fabsf(py - bx[1]), fabsf(py - bx[4]));
    if (pz < bx[2] || pz > bx[5]) dz = fminf(fabsf(pz - bx[2]), fabsf(pz - bx[5]));
    return fma_(dz, dz, fma_(dy, dy, dx * dx));
}

__device__ __forceinline__ float bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

}  // namespace
