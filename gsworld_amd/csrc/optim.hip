// optim.hip -- the optimizer step and the densification statistics of a training iteration (gsr_adam_update,
// gsr_densification_stats; include/gsr.h holds the definitions, evaluation order included).
//
// adam_kernel: ONE launch for all parameter groups of a step.  A group is (N, M) float32; its N * M elements are cut into
// work units, one per thread, 256 per workgroup, and every group owns a contiguous range of workgroups (AdamArgs::block0).
//   * a group whose four arrays are 16-byte aligned: a unit is the float4 at elements 4 q .. 4 q + 3.  The unit walks its
//     (up to four) Gaussians once and reads one visibility word per Gaussian; all four elements visible -> four float4
//     loads, three float4 stores; none visible -> nothing but the visibility word is read; mixed (a vector that straddles
//     Gaussians of different visibility: every M that is no multiple of 4 -- or the ragged last vector) -> the visible
//     elements one by one, nothing else read or written.
//   * any other group: a unit is one element.
// Element indices are 64-bit.  Invisible Gaussians cost no load of grad / exp_avg / exp_avg_sq (and none of param).
// The arithmetic is written operation by operation; the library builds with -ffp-contract=off, `/` and sqrtf are the
// correctly rounded binary32 ones, denormals kept.
//
// stats_kernel: one thread per Gaussian.
//
// No allocation, no synchronisation: both calls can be captured into a hipGraph (the captured lr is replayed).
#include "gsr_internal.h"

#include <string.h>

namespace {

constexpr int kOptBlock = 256;

struct AdamGroupArgs {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t total;   // N * M
    int64_t block0;  // first workgroup of this group
    int32_t M;
    int32_t vec;  // 1: float4 units
    float nlr, b1, omb1, b2, omb2, eps;
};

struct AdamArgs {
    AdamGroupArgs grp[GSR_ADAM_MAX_GROUPS];
    const void *visible;
    int32_t kind;
    int32_t num_groups;
};

__device__ __forceinline__ bool is_visible(const void *vis, int kind, int64_t row) {
    if (kind == GSR_VISIBLE_MASK8) return ((const uint8_t *)vis)[row] != 0;
    if (kind == GSR_VISIBLE_RADII) return ((const int32_t *)vis)[row] > 0;
    return true;
}

// include/gsr.h: m' = (b1 m) + ((1 - b1) g); v' = (b2 v) + (((1 - b2) g) g); p' = p + ((-lr m') / (sqrtf(v') + eps))
__device__ __forceinline__ void adam_one(const AdamGroupArgs &a, float &p, float g, float &m, float &v) {
    const float t0 = a.b1 * m;
    const float t1 = a.omb1 * g;
    m = t0 + t1;
    const float u0 = a.b2 * v;
    const float u1 = a.omb2 * g;
    const float u2 = u1 * g;
    v = u0 + u2;
    const float num = a.nlr * m;
    const float den = sqrtf(v) + a.eps;
    p = p + num / den;
}

__global__ __launch_bounds__(kOptBlock) void adam_kernel(const AdamArgs a) {
    // this workgroup's group: the last one whose range starts at or before it (static indices: the arguments stay in SGPRs)
    const int64_t blk = (int64_t)blockIdx.x;
    AdamGroupArgs G = a.grp[0];
#pragma unroll
    for (int k = 1; k < GSR_ADAM_MAX_GROUPS; k++)
        if (k < a.num_groups && blk >= a.grp[k].block0) G = a.grp[k];
    const int64_t unit = (blk - G.block0) * kOptBlock + threadIdx.x;
    const int kind = a.kind;
    if (!G.vec) {
        if (unit >= G.total) return;
        if (!is_visible(a.visible, kind, unit / G.M)) return;
        float p = G.p[unit], m = G.m[unit], v = G.v[unit];
        adam_one(G, p, G.g[unit], m, v);
        G.p[unit] = p;
        G.m[unit] = m;
        G.v[unit] = v;
        return;
    }
    const int64_t e0 = unit * 4;
    if (e0 >= G.total) return;
    int64_t row = e0 / G.M;
    int32_t off = (int32_t)(e0 - row * G.M);
    const int valid = G.total - e0 >= 4 ? 4 : (int)(G.total - e0);
    bool cur = is_visible(a.visible, kind, row);
    bool vis[4];
    int nvis = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j < valid) {
            if (off == G.M) {  // (never taken at j == 0: off < M there)
                off = 0;
                row++;
                cur = is_visible(a.visible, kind, row);
            }
            off++;
        }
        vis[j] = j < valid && cur;
        nvis += vis[j] ? 1 : 0;
    }
    if (nvis == 0) return;
    if (nvis == 4) {
        float4 p = *reinterpret_cast<const float4 *>(G.p + e0);
        const float4 g = *reinterpret_cast<const float4 *>(G.g + e0);
        float4 m = *reinterpret_cast<const float4 *>(G.m + e0);
        float4 v = *reinterpret_cast<const float4 *>(G.v + e0);
        adam_one(G, p.x, g.x, m.x, v.x);
        adam_one(G, p.y, g.y, m.y, v.y);
        adam_one(G, p.z, g.z, m.z, v.z);
        adam_one(G, p.w, g.w, m.w, v.w);
        *reinterpret_cast<float4 *>(G.p + e0) = p;
        *reinterpret_cast<float4 *>(G.m + e0) = m;
        *reinterpret_cast<float4 *>(G.v + e0) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!vis[j]) continue;
        const int64_t e = e0 + j;
        float p = G.p[e], m = G.m[e], v = G.v[e];
        adam_one(G, p, G.g[e], m, v);
        G.p[e] = p;
        G.m[e] = m;
        G.v[e] = v;
    }
}

__global__ __launch_bounds__(kOptBlock) void stats_kernel(int32_t N, const int32_t *__restrict__ radii,
                                                          const float *__restrict__ grad2D, float *__restrict__ accum,
                                                          float *__restrict__ denom, float *__restrict__ max_radii) {
    const int64_t i = (int64_t)blockIdx.x * kOptBlock + threadIdx.x;
    if (i >= N) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    const float gx = grad2D[3 * i], gy = grad2D[3 * i + 1];
    const float xx = gx * gx;
    const float yy = gy * gy;
    const float s = xx + yy;
    accum[i] = accum[i] + sqrtf(s);
    denom[i] = denom[i] + 1.0f;
    if (max_radii) max_radii[i] = fmaxf(max_radii[i], (float)r);
}

}  // namespace

extern "C" int gsr_adam_update(const GsrAdamStep *s, void *stream) {
    if (!s) {
        gsr_set_error("gsr_adam_update: null step");
        return GSR_E_INVALID;
    }
    if (s->struct_size != (int32_t)sizeof(GsrAdamStep)) {
        gsr_set_error("gsr_adam_update: struct_size %d, this library's GsrAdamStep has %d bytes", (int)s->struct_size,
                      (int)sizeof(GsrAdamStep));
        return GSR_E_INVALID;
    }
    if (s->N < 0) {
        gsr_set_error("gsr_adam_update: N = %d", (int)s->N);
        return GSR_E_INVALID;
    }
    if (s->num_groups < 1 || s->num_groups > GSR_ADAM_MAX_GROUPS) {
        gsr_set_error("gsr_adam_update: need 1 <= num_groups <= %d, got %d", GSR_ADAM_MAX_GROUPS, (int)s->num_groups);
        return GSR_E_INVALID;
    }
    if (s->visible_kind != GSR_VISIBLE_ALL && s->visible_kind != GSR_VISIBLE_MASK8 && s->visible_kind != GSR_VISIBLE_RADII) {
        gsr_set_error("gsr_adam_update: visible_kind %d", (int)s->visible_kind);
        return GSR_E_INVALID;
    }
    if ((s->visible_kind == GSR_VISIBLE_ALL) != (s->visible == nullptr)) {
        gsr_set_error("gsr_adam_update: visible_kind %d with a %s `visible`", (int)s->visible_kind,
                      s->visible ? "non-null" : "null");
        return GSR_E_INVALID;
    }
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    int64_t blocks = 0;
    for (int k = 0; k < s->num_groups; k++) {
        const GsrAdamGroup &g = s->groups[k];
        if (g.M < 1 || g.M > 4096) {
            gsr_set_error("gsr_adam_update: group %d: need 1 <= M <= 4096, got %d", k, (int)g.M);
            return GSR_E_INVALID;
        }
        if (s->N > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)) {
            gsr_set_error("gsr_adam_update: group %d: null param, grad, exp_avg or exp_avg_sq", k);
            return GSR_E_INVALID;
        }
        AdamGroupArgs &o = a.grp[k];
        o.p = g.param;
        o.g = g.grad;
        o.m = g.exp_avg;
        o.v = g.exp_avg_sq;
        o.total = (int64_t)s->N * g.M;
        o.block0 = blocks;
        o.M = g.M;
        o.vec = (((uintptr_t)g.param | (uintptr_t)g.grad | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq) & 15) == 0;
        o.nlr = -g.lr;
        o.b1 = g.beta1;
        o.omb1 = 1.0f - g.beta1;
        o.b2 = g.beta2;
        o.omb2 = 1.0f - g.beta2;
        o.eps = g.eps;
        const int64_t units = o.vec ? (o.total + 3) / 4 : o.total;
        blocks += (units + kOptBlock - 1) / kOptBlock;
    }
    if (s->N == 0) return GSR_OK;
    if (blocks > 0x7fffffffLL) {
        gsr_set_error("gsr_adam_update: %lld workgroups exceed one launch", (long long)blocks);
        return GSR_E_INVALID;
    }
    a.visible = s->visible;
    a.kind = s->visible_kind;
    a.num_groups = s->num_groups;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(kOptBlock), 0, (hipStream_t)stream, a);
    return gsr_check_launch("adam_update", false, (hipStream_t)stream);
}

extern "C" int gsr_densification_stats(int32_t N, const int32_t *radii, const float *grad_means2D, float *grad_accum,
                                       float *denom, float *max_radii2D, void *stream) {
    if (N < 0) {
        gsr_set_error("gsr_densification_stats: N = %d", (int)N);
        return GSR_E_INVALID;
    }
    if (N == 0) return GSR_OK;
    if (!radii || !grad_means2D || !grad_accum || !denom) {
        gsr_set_error("gsr_densification_stats: null radii, grad_means2D, grad_accum or denom");
        return GSR_E_INVALID;
    }
    hipLaunchKernelGGL(stats_kernel, dim3(gsr_div_up(N, kOptBlock)), dim3(kOptBlock), 0, (hipStream_t)stream, N, radii,
                       grad_means2D, grad_accum, denom, max_radii2D);
    return gsr_check_launch("densification_stats", false, (hipStream_t)stream);
}
