// densify.hip -- densify-and-prune of the Gaussian model on the device (gsr_densify_plan, gsr_densify_apply; include/gsr.h
// holds the definition, evaluation order included).  Upstream's densify_and_clone -> densify_and_split -> prune_points
// sequence as two calls, so that the data-dependent output size crosses to the host once, between them.
//
// gsr_densify_plan, three launches with plain launch boundaries between them (no ticket, no last-workgroup tail):
//   decide_kernel   one thread per Gaussian: the three flags (self kept, clone emitted, children emitted) into one byte
//                   of the workspace, and the workgroup's count of each flag.
//   blockscan_kernel ONE workgroup: exclusive running sums of the workgroup counts, 256 at a time with a carry; the
//                   totals become counts[4] (caller's array and the workspace header).
//   place_kernel    one thread per Gaussian: workgroup base + a workgroup-local scan of the flags (the three 0/1 streams
//                   packed into one word, 10 bits each) = the Gaussian's slot in each segment; it writes its own index
//                   there: the workspace's row map (output row -> parent), four ascending segments.
// gsr_densify_apply, ONE launch: every group's param / exp_avg / exp_avg_sq, and the parent output.  Threads map to OUTPUT
// elements; each group owns a contiguous range of workgroups (as adam_kernel's groups do), a unit is the float4 at
// destination elements 4 q .. 4 q + 3 when the group's destinations are 16-byte aligned, else one element.  Sources are
// read through the row map.  Which segment a row is in follows from the counts in the workspace header.
//
// Gaussian indices are 32-bit (N <= 2^30), element indices 64-bit.  expf / logf are the <= 1 ulp library ones; the
// library builds with -ffp-contract=off.  No allocation, no synchronisation.
#include "gsr_internal.h"

#include <string.h>

namespace {

constexpr int kBlock = 256;
constexpr int kHeaderBytes = 256;
constexpr uint32_t kKeep = 1u, kClone = 2u, kSplit = 4u;

struct Workspace {
    int32_t *header;    // [0..3] = counts
    uint32_t *blocks;   // 3 per workgroup of decide_kernel: kept, clones, splits (counts, then exclusive sums)
    uint8_t *flags;     // N
    int32_t *rowmap;    // 2 N: output row -> parent
    static size_t bytes(int64_t N) {
        const int64_t nb = (N + kBlock - 1) / kBlock;
        return (size_t)kHeaderBytes + gsr_align_up((size_t)nb * 3 * sizeof(uint32_t)) + gsr_align_up((size_t)N) +
               gsr_align_up((size_t)N * 2 * sizeof(int32_t));
    }
    Workspace(void *base, int64_t N) {
        const int64_t nb = (N + kBlock - 1) / kBlock;
        char *p = (char *)base;
        header = (int32_t *)p;
        p += kHeaderBytes;
        blocks = (uint32_t *)p;
        p += gsr_align_up((size_t)nb * 3 * sizeof(uint32_t));
        flags = (uint8_t *)p;
        p += gsr_align_up((size_t)N);
        rowmap = (int32_t *)p;
    }
};

// max that propagates NaN (torch.max; fmaxf drops it)
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

__global__ __launch_bounds__(kBlock) void decide_kernel(int32_t N, const float *__restrict__ accum,
                                                        const float *__restrict__ denom, const float *__restrict__ scaling,
                                                        const float *__restrict__ opacity, float grad_threshold,
                                                        float min_opacity, float dense_limit, float world_limit,
                                                        int world_on, uint8_t *__restrict__ flags,
                                                        uint32_t *__restrict__ blocks) {
    __shared__ uint32_t s_w[4];
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    uint32_t f = 0;
    if (i < N) {
        float g = accum[i] / denom[i];
        if (g != g) g = 0.0f;
        const bool hot_clone = fabsf(g) >= grad_threshold;
        const bool hot_split = g >= grad_threshold;
        const float e0 = expf(scaling[3 * (int64_t)i]), e1 = expf(scaling[3 * (int64_t)i + 1]),
                    e2 = expf(scaling[3 * (int64_t)i + 2]);
        const float smax = nan_max(nan_max(e0, e1), e2);
        const bool small = smax <= dense_limit;
        const bool clone_sel = hot_clone && small;
        const bool split_sel = hot_split && !small;
        const float en = expf(-opacity[i]);
        const float op = 1.0f / (1.0f + en);
        const bool prune_op = op < min_opacity;
        const bool big_self = world_on && smax > world_limit;
        const float c0 = expf(logf(e0 / 1.6f)), c1 = expf(logf(e1 / 1.6f)), c2 = expf(logf(e2 / 1.6f));
        const bool big_child = world_on && nan_max(nan_max(c0, c1), c2) > world_limit;
        if (!split_sel && !prune_op && !big_self) f |= kKeep;
        if (clone_sel && !prune_op && !big_self) f |= kClone;
        if (split_sel && !prune_op && !big_child) f |= kSplit;
        flags[i] = (uint8_t)f;
    }
    uint32_t total;
    gsr_block_incl_scan((f & 1u) | ((f >> 1 & 1u) << 10) | ((f >> 2 & 1u) << 20), s_w, total);
    if (threadIdx.x == 0) {
        blocks[3 * (int64_t)blockIdx.x] = total & 1023u;
        blocks[3 * (int64_t)blockIdx.x + 1] = total >> 10 & 1023u;
        blocks[3 * (int64_t)blockIdx.x + 2] = total >> 20 & 1023u;
    }
}

__global__ __launch_bounds__(kBlock) void blockscan_kernel(int32_t nb, uint32_t *__restrict__ blocks,
                                                           int32_t *__restrict__ header, int32_t *__restrict__ counts) {
    __shared__ uint32_t s_w[4];
    uint32_t carry[3] = {0u, 0u, 0u};
    for (int32_t base = 0; base < nb; base += kBlock) {
        const int32_t b = base + (int32_t)threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t c = b < nb ? blocks[3 * (int64_t)b + k] : 0u;
            uint32_t total;
            const uint32_t incl = gsr_block_incl_scan(c, s_w, total);
            if (b < nb) blocks[3 * (int64_t)b + k] = carry[k] + incl - c;
            carry[k] += total;
        }
    }
    if (threadIdx.x == 0) {
        const int32_t out[4] = {(int32_t)carry[0], (int32_t)carry[1], (int32_t)carry[2],
                                (int32_t)(carry[0] + carry[1] + 2u * carry[2])};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            header[k] = out[k];
            counts[k] = out[k];
        }
    }
}

__global__ __launch_bounds__(kBlock) void place_kernel(int32_t N, const uint8_t *__restrict__ flags,
                                                       const uint32_t *__restrict__ blocks,
                                                       const int32_t *__restrict__ header, int32_t *__restrict__ rowmap) {
    __shared__ uint32_t s_w[4];
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const uint32_t f = i < N ? flags[i] : 0u;
    const uint32_t v = (f & 1u) | ((f >> 1 & 1u) << 10) | ((f >> 2 & 1u) << 20);
    uint32_t total;
    const uint32_t excl = gsr_block_incl_scan(v, s_w, total) - v;
    const uint32_t K = (uint32_t)header[0], Cn = (uint32_t)header[1], S = (uint32_t)header[2];
    if (f & kKeep) rowmap[blocks[3 * (int64_t)blockIdx.x] + (excl & 1023u)] = i;
    if (f & kClone) rowmap[K + blocks[3 * (int64_t)blockIdx.x + 1] + (excl >> 10 & 1023u)] = i;
    if (f & kSplit) {
        const uint32_t at = K + Cn + blocks[3 * (int64_t)blockIdx.x + 2] + (excl >> 20 & 1023u);
        rowmap[at] = i;
        rowmap[at + S] = i;
    }
}

struct ApplyGroupArgs {
    const float *sp, *sm, *sv;
    float *dp, *dm, *dv;
    int64_t total;   // N_out * M
    int64_t block0;  // first workgroup of this group
    int32_t M;
    int32_t vec;  // 1: float4 units
    int32_t role;
    int32_t pad;
};

struct ApplyArgs {
    ApplyGroupArgs grp[GSR_ADAM_MAX_GROUPS];
    const int32_t *rowmap;
    const int32_t *header;
    const float *xyz, *scaling, *rotation, *noise;
    int32_t *parent;
    int64_t pblock0;  // first workgroup of the parent output
    int32_t num_groups;
    int32_t N_out;
};

// component k of a child's position: (R_k0 v0 + R_k1 v1) + R_k2 v2, then + xyz_k, v[j] = expf(s[j]) * noise[par][c][j],
// R = build_rotation of the parent's raw quaternion (normalised first, its nine entries as that function writes them)
__device__ __forceinline__ float child_position(const ApplyArgs &a, int32_t par, int c, int k) {
    const float *s = a.scaling + 3 * (int64_t)par;
    const float *n = a.noise + 6 * (int64_t)par + 3 * c;
    const float v0 = expf(s[0]) * n[0], v1 = expf(s[1]) * n[1], v2 = expf(s[2]) * n[2];
    const float *r = a.rotation + 4 * (int64_t)par;
    const float rw = r[0], rx = r[1], ry = r[2], rz = r[3];
    const float norm = sqrtf(((rw * rw + rx * rx) + ry * ry) + rz * rz);
    const float w = rw / norm, x = rx / norm, y = ry / norm, z = rz / norm;
    float r0, r1, r2;
    if (k == 0) {
        r0 = 1.0f - 2.0f * (y * y + z * z);
        r1 = 2.0f * (x * y - w * z);
        r2 = 2.0f * (x * z + w * y);
    } else if (k == 1) {
        r0 = 2.0f * (x * y + w * z);
        r1 = 1.0f - 2.0f * (x * x + z * z);
        r2 = 2.0f * (y * z - w * x);
    } else {
        r0 = 2.0f * (x * z - w * y);
        r1 = 2.0f * (y * z + w * x);
        r2 = 1.0f - 2.0f * (x * x + y * y);
    }
    const float t = (r0 * v0 + r1 * v1) + r2 * v2;
    return t + a.xyz[3 * (int64_t)par + k];
}

__device__ __forceinline__ void apply_one(const ApplyArgs &a, const ApplyGroupArgs &G, int64_t row, int32_t col, uint32_t K,
                                          uint32_t KC, uint32_t KCS, float &p, float &m, float &v) {
    const int32_t par = a.rowmap[row];
    const int64_t src = (int64_t)par * G.M + col;
    m = 0.0f;
    v = 0.0f;
    if ((uint64_t)row < K) {  // a kept self: parameter and moments bit for bit
        p = G.sp[src];
        if (G.sm) {
            m = G.sm[src];
            v = G.sv[src];
        }
    } else if ((uint64_t)row < KC || G.role == GSR_DENSIFY_COPY) {
        p = G.sp[src];
    } else if (G.role == GSR_DENSIFY_SCALING) {
        p = logf(expf(G.sp[src]) / 1.6f);
    } else {
        p = child_position(a, par, (uint64_t)row >= KCS ? 1 : 0, col);
    }
}

__global__ __launch_bounds__(kBlock) void apply_kernel(const ApplyArgs a) {
    const int64_t blk = (int64_t)blockIdx.x;
    const uint32_t K = (uint32_t)a.header[0], KC = K + (uint32_t)a.header[1], KCS = KC + (uint32_t)a.header[2];
    // (a caller whose N_out is larger than the plan's writes the plan's rows only: the row map holds no more)
    const int64_t rows = min((int64_t)a.N_out, (int64_t)KCS + (int64_t)a.header[2]);
    if (blk >= a.pblock0) {
        const int64_t r = (blk - a.pblock0) * kBlock + threadIdx.x;
        if (r < rows) a.parent[r] = a.rowmap[r];
        return;
    }
    ApplyGroupArgs G = a.grp[0];
#pragma unroll
    for (int k = 1; k < GSR_ADAM_MAX_GROUPS; k++)
        if (k < a.num_groups && blk >= a.grp[k].block0) G = a.grp[k];
    const int64_t unit = (blk - G.block0) * kBlock + threadIdx.x;
    const int64_t total = min(G.total, rows * G.M);
    if (!G.vec) {
        if (unit >= total) return;
        const int64_t row = unit / G.M;
        float p, m, v;
        apply_one(a, G, row, (int32_t)(unit - row * G.M), K, KC, KCS, p, m, v);
        G.dp[unit] = p;
        if (G.dm) {
            G.dm[unit] = m;
            G.dv[unit] = v;
        }
        return;
    }
    const int64_t e0 = unit * 4;
    if (e0 >= total) return;
    int64_t row = e0 / G.M;
    int32_t col = (int32_t)(e0 - row * G.M);
    const int valid = total - e0 >= 4 ? 4 : (int)(total - e0);
    float p[4], m[4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p[j] = m[j] = v[j] = 0.0f;
        if (j < valid) {
            if (col == G.M) {
                col = 0;
                row++;
            }
            apply_one(a, G, row, col, K, KC, KCS, p[j], m[j], v[j]);
            col++;
        }
    }
    if (valid == 4) {
        *reinterpret_cast<float4 *>(G.dp + e0) = make_float4(p[0], p[1], p[2], p[3]);
        if (G.dm) {
            *reinterpret_cast<float4 *>(G.dm + e0) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(G.dv + e0) = make_float4(v[0], v[1], v[2], v[3]);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j >= valid) continue;
        G.dp[e0 + j] = p[j];
        if (G.dm) {
            G.dm[e0 + j] = m[j];
            G.dv[e0 + j] = v[j];
        }
    }
}

struct Range {
    uintptr_t lo, hi;
};
inline bool overlap(const Range &a, const Range &b) { return a.lo < b.hi && b.lo < a.hi && a.lo < a.hi && b.lo < b.hi; }

}  // namespace

extern "C" int64_t gsr_densify_workspace_bytes(int32_t N) {
    if (N < 0) N = 0;
    return (int64_t)Workspace::bytes(N);
}

extern "C" int gsr_densify_plan(const GsrDensifyPlan *s, void *stream) {
    if (!s) {
        gsr_set_error("gsr_densify_plan: null plan");
        return GSR_E_INVALID;
    }
    if (s->struct_size != (int32_t)sizeof(GsrDensifyPlan)) {
        gsr_set_error("gsr_densify_plan: struct_size %d, this library's GsrDensifyPlan has %d bytes", (int)s->struct_size,
                      (int)sizeof(GsrDensifyPlan));
        return GSR_E_INVALID;
    }
    if (s->N < 0 || s->N > (1 << 30)) {
        gsr_set_error("gsr_densify_plan: N = %d (0 .. 2^30)", (int)s->N);
        return GSR_E_INVALID;
    }
    if (s->N == 0) return GSR_OK;
    if (!s->grad_accum || !s->denom || !s->scaling || !s->opacity || !s->counts || !s->workspace) {
        gsr_set_error("gsr_densify_plan: null grad_accum, denom, scaling, opacity, counts or workspace");
        return GSR_E_INVALID;
    }
    if (s->workspace_bytes < gsr_densify_workspace_bytes(s->N)) {
        gsr_set_error("gsr_densify_plan: workspace of %lld bytes, %lld needed for N = %d", (long long)s->workspace_bytes,
                      (long long)gsr_densify_workspace_bytes(s->N), (int)s->N);
        return GSR_E_INVALID;
    }
    if (((uintptr_t)s->workspace & 15) || ((uintptr_t)s->counts & 3)) {
        gsr_set_error("gsr_densify_plan: workspace must be 16-byte aligned, counts 4-byte aligned");
        return GSR_E_INVALID;
    }
    const Workspace w(s->workspace, s->N);
    const int nb = gsr_div_up(s->N, kBlock);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decide_kernel, dim3(nb), dim3(kBlock), 0, st, s->N, s->grad_accum, s->denom, s->scaling, s->opacity,
                       s->grad_threshold, s->min_opacity, s->dense_limit, s->world_limit, s->prune_world_size != 0 ? 1 : 0,
                       w.flags, w.blocks);
    hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(kBlock), 0, st, nb, w.blocks, w.header, s->counts);
    hipLaunchKernelGGL(place_kernel, dim3(nb), dim3(kBlock), 0, st, s->N, w.flags, w.blocks, w.header, w.rowmap);
    return gsr_check_launch("densify_plan", false, st);
}

extern "C" int gsr_densify_apply(const GsrDensifyApply *s, void *stream) {
    if (!s) {
        gsr_set_error("gsr_densify_apply: null arguments");
        return GSR_E_INVALID;
    }
    if (s->struct_size != (int32_t)sizeof(GsrDensifyApply)) {
        gsr_set_error("gsr_densify_apply: struct_size %d, this library's GsrDensifyApply has %d bytes", (int)s->struct_size,
                      (int)sizeof(GsrDensifyApply));
        return GSR_E_INVALID;
    }
    if (s->N < 0 || s->N > (1 << 30)) {
        gsr_set_error("gsr_densify_apply: N = %d (0 .. 2^30)", (int)s->N);
        return GSR_E_INVALID;
    }
    if (s->N == 0) return GSR_OK;
    if (s->N_out < 0 || (int64_t)s->N_out > 2 * (int64_t)s->N) {
        gsr_set_error("gsr_densify_apply: N_out = %d (0 .. 2 N = %lld)", (int)s->N_out, 2 * (long long)s->N);
        return GSR_E_INVALID;
    }
    if (s->num_groups < 0 || s->num_groups > GSR_ADAM_MAX_GROUPS) {
        gsr_set_error("gsr_densify_apply: need 0 <= num_groups <= %d, got %d", GSR_ADAM_MAX_GROUPS, (int)s->num_groups);
        return GSR_E_INVALID;
    }
    if (!s->workspace || !s->xyz || !s->scaling || !s->rotation || !s->noise || (!s->parent && s->N_out > 0)) {
        gsr_set_error("gsr_densify_apply: null workspace, xyz, scaling, rotation, noise or parent");
        return GSR_E_INVALID;
    }
    if (s->workspace_bytes < gsr_densify_workspace_bytes(s->N) || ((uintptr_t)s->workspace & 15)) {
        gsr_set_error("gsr_densify_apply: workspace of %lld bytes (%lld needed for N = %d), or not 16-byte aligned",
                      (long long)s->workspace_bytes, (long long)gsr_densify_workspace_bytes(s->N), (int)s->N);
        return GSR_E_INVALID;
    }
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    Range src[3 * GSR_ADAM_MAX_GROUPS + 5], dst[3 * GSR_ADAM_MAX_GROUPS + 1];
    int ns = 0, nd = 0;
    auto add = [](Range *r, int &n, const void *p, int64_t bytes) {
        if (p && bytes > 0) r[n++] = Range{(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes};
    };
    add(src, ns, s->workspace, gsr_densify_workspace_bytes(s->N));
    add(src, ns, s->xyz, (int64_t)s->N * 12);
    add(src, ns, s->scaling, (int64_t)s->N * 12);
    add(src, ns, s->rotation, (int64_t)s->N * 16);
    add(src, ns, s->noise, (int64_t)s->N * 24);
    add(dst, nd, s->parent, (int64_t)s->N_out * 4);
    int64_t blocks = 0;
    for (int k = 0; k < s->num_groups; k++) {
        const GsrDensifyGroup &g = s->groups[k];
        if (g.M < 1 || g.M > 4096) {
            gsr_set_error("gsr_densify_apply: group %d: need 1 <= M <= 4096, got %d", k, (int)g.M);
            return GSR_E_INVALID;
        }
        if (g.role != GSR_DENSIFY_COPY && g.role != GSR_DENSIFY_XYZ && g.role != GSR_DENSIFY_SCALING) {
            gsr_set_error("gsr_densify_apply: group %d: role %d", k, (int)g.role);
            return GSR_E_INVALID;
        }
        if (g.role != GSR_DENSIFY_COPY && g.M != 3) {
            gsr_set_error("gsr_densify_apply: group %d: the xyz and scaling roles have M = 3, got %d", k, (int)g.M);
            return GSR_E_INVALID;
        }
        if (!g.param || (!g.out_param && s->N_out > 0)) {
            gsr_set_error("gsr_densify_apply: group %d: null param or out_param", k);
            return GSR_E_INVALID;
        }
        const bool moments = g.exp_avg != nullptr;
        if ((g.exp_avg_sq != nullptr) != moments ||
            (s->N_out > 0 && ((g.out_exp_avg != nullptr) != moments || (g.out_exp_avg_sq != nullptr) != moments))) {
            gsr_set_error("gsr_densify_apply: group %d: exp_avg, exp_avg_sq and their outputs are all given or all null", k);
            return GSR_E_INVALID;
        }
        const int64_t sb = (int64_t)s->N * g.M * 4, db = (int64_t)s->N_out * g.M * 4;
        add(src, ns, g.param, sb);
        add(src, ns, g.exp_avg, sb);
        add(src, ns, g.exp_avg_sq, sb);
        add(dst, nd, g.out_param, db);
        add(dst, nd, g.out_exp_avg, db);
        add(dst, nd, g.out_exp_avg_sq, db);
        ApplyGroupArgs &o = a.grp[k];
        o.sp = g.param;
        o.sm = g.exp_avg;
        o.sv = g.exp_avg_sq;
        o.dp = g.out_param;
        o.dm = moments ? g.out_exp_avg : nullptr;
        o.dv = moments ? g.out_exp_avg_sq : nullptr;
        o.total = (int64_t)s->N_out * g.M;
        o.block0 = blocks;
        o.M = g.M;
        o.role = g.role;
        o.vec = (((uintptr_t)o.dp | (uintptr_t)o.dm | (uintptr_t)o.dv) & 15) == 0;
        const int64_t units = o.vec ? (o.total + 3) / 4 : o.total;
        blocks += (units + kBlock - 1) / kBlock;
    }
    for (int i = 0; i < nd; i++) {
        for (int j = 0; j < ns; j++)
            if (overlap(dst[i], src[j])) {
                gsr_set_error("gsr_densify_apply: an output overlaps an input (or the workspace)");
                return GSR_E_INVALID;
            }
        for (int j = i + 1; j < nd; j++)
            if (overlap(dst[i], dst[j])) {
                gsr_set_error("gsr_densify_apply: two outputs overlap");
                return GSR_E_INVALID;
            }
    }
    if (s->N_out == 0) return GSR_OK;
    a.pblock0 = blocks;
    blocks += ((int64_t)s->N_out + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) {
        gsr_set_error("gsr_densify_apply: %lld workgroups exceed one launch", (long long)blocks);
        return GSR_E_INVALID;
    }
    const Workspace w(const_cast<void *>(s->workspace), s->N);
    a.rowmap = w.rowmap;
    a.header = w.header;
    a.xyz = s->xyz;
    a.scaling = s->scaling;
    a.rotation = s->rotation;
    a.noise = s->noise;
    a.parent = s->parent;
    a.num_groups = s->num_groups;
    a.N_out = s->N_out;
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
    return gsr_check_launch("densify_apply", false, (hipStream_t)stream);
}
