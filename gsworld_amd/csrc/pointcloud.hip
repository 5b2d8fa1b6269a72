// pointcloud.hip -- point-cloud observations of the splatted scene (gsr_render_pointcloud, include/gsr.h).
//
// Definition (the contract of every layer above and of tests/test_pointcloud_*.py).  Per environment e and camera c the
// inputs are the depth map D and label map L of gsr_render_maps (with the depth_scale they were written with), the uint8
// frame, the camera's view matrix (GsrInputs.viewmatrix: W2C^T, 16 floats, W2C[r][k] = m[4k + r]) and tanfovx / tanfovy.
// All arithmetic is binary32 in the order written, no contraction (the library builds with -ffp-contract=off):
//   * a pixel is a point when D[y,x] > 0 (the maps write exactly 0.0 for background and for every pixel of an overflowed
//     frame);
//   * z = D / depth_scale; ndc_x = (float)(2x+1) / (float)W - 1, ndc_y = (float)(2y+1) / (float)H - 1 (the inverse of the
//     preprocess's ndc2Pix); xv = (ndc_x tanfovx) z, yv = (ndc_y tanfovy) z, zv = z;
//   * p = C2W (xv, yv, zv, 1) row by row as ((m0 xv + m1 yv) + m2 zv) + m3, then q = A p the same way with the caller's
//     3 x 4 out_from_scene A.  C2W is computed once per frame in binary64 from a = W2C[:3,:3], t = W2C[:3,3]:
//       c00 = a11 a22 - a12 a21,  c01 = a12 a20 - a10 a22,  c02 = a10 a21 - a11 a20,  det = (a00 c00 + a01 c01) + a02 c02
//       R0 = (c00, a02 a21 - a01 a22, a01 a12 - a02 a11) / det
//       R1 = (c01, a00 a22 - a02 a20, a02 a10 - a00 a12) / det
//       R2 = (c02, a01 a20 - a00 a21, a00 a11 - a01 a10) / det
//       t'_i = -((Ri0 t0 + Ri1 t1) + Ri2 t2)
//     and every entry rounded to binary32 (row i of C2W = (Ri0, Ri1, Ri2, t'_i));
//   * a point is VALID when q lies inside the optional crop box [lo, hi] (inclusive) and its label is not in the optional
//     exclusion bitmap (bit (uint16)label);
//   * within an environment points are ordered camera by camera, then row-major by pixel;
//   * payload of a valid point: xyzw = (q, 1), rgb = the frame's pixel, segmentation = L[y,x] (-1 without a label map);
//     an invalid or unused slot holds xyzw = 0, rgb = 0, segmentation = -1.
// Modes: DENSE (one slot per pixel, count = valid points), STRIDE (slot j < M = min(n, K) holds the valid point of rank
// floor(j n / M)), FPS (the same selection with M = min(n, fps_candidates) gives the candidates; farthest-point sampling
// from candidate 0 with d = ((dx dx) + (dy dy)) + dz dz, dmin <- d < dmin ? d : dmin, argmax with ties to the lowest index,
// min(M, K) picks in pick order).
//
// Launches (one stream, no allocation, no host synchronisation: capturable):
//   1. pc_pixel_kernel: grid (blocks of the largest frame, E C frames), 256 pixels per workgroup.  Unprojects, crops,
//      filters; per-workgroup valid counts by ballot + popcount (deterministic); DENSE writes its slots here.
//   2. pc_scan_kernel: one workgroup per environment: the counts of its workgroups (camera by camera, in pixel order) become
//      exclusive offsets in place, n and count[e] are written; STRIDE clears its unused slots.
//   3. pc_select_kernel (STRIDE, FPS): the pixel pass again, now with the rank of every valid point (offset + ballot/mbcnt
//      rank); the point whose rank is floor(j n / M) goes to slot j -- of the output (STRIDE) or of the candidate workspace
//      (FPS).  Slot j of rank r exists iff j = ceil(r M / n) < M and floor(j n / M) = r (n >= M: the map is injective).
//   4. pc_fps_kernel (FPS): one 1024-thread workgroup per environment; candidate i lives in lane i % 1024, register
//      i / 1024 (coordinates and running dmin in VGPRs).  Per pick every lane updates its dmin and keeps its best
//      (d > best: the lowest index wins ties), the wave takes the max of 64-bit keys (float_bits(dmin) << 32 | ~index) in
//      DPP moves, its winner writes key and coordinates to one LDS slot per wave (double-buffered: one barrier per pick),
//      and every thread reduces the 16 slots.  Picks are written out in a final parallel pass.
#include "gsr_internal.h"

#include <float.h>
#include <string.h>

namespace {

constexpr int kPcBlock = 256;
constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / GSR_WAVE;

struct PcView {
    const float *vm;        // device, 16 floats (W2C^T)
    const float *depth;     // (H,W)
    const int16_t *label;   // (H,W) or nullptr
    const uint8_t *rgb;     // (H,W,3) or nullptr
    int W, H;
    float tanfovx, tanfovy, depth_scale;
    int pad;
};

struct PcArgs {
    PcView v[GSR_PC_MAX_VIEWS];
    float A[12];
    float lo[3], hi[3];
    int crop;
    const uint32_t *excl;   // 2048 words or nullptr
    float4 *xyzw;           // (E, N, 4)
    uint8_t *rgb;           // (E, N, 3)
    int16_t *seg;           // (E, N)
    int32_t *count;         // (E)
    int32_t *blk;           // (E, NB): per-workgroup valid counts, then exclusive offsets
    int32_t *env_n;         // (E)
    float4 *cand;           // (E, Mcap): (q, rgb bits)
    int16_t *cand_seg;      // (E, Mcap)
    int E, C, NB, N, mode, K, Mcap;
};
static_assert(sizeof(PcArgs) <= 4096 - 128, "the point-cloud arguments must fit the 4 KiB kernarg segment");

__device__ __forceinline__ void pc_c2w(const float *m, float *out) {
    const double a[3][3] = {{m[0], m[4], m[8]}, {m[1], m[5], m[9]}, {m[2], m[6], m[10]}};
    const double t0 = m[12], t1 = m[13], t2 = m[14];
    double r[3][3];
    gsr_inverse3_f64(a, r);  // (gsr_internal.h: the cofactor formula below)
    for (int i = 0; i < 3; i++) {
        out[4 * i + 0] = (float)r[i][0];
        out[4 * i + 1] = (float)r[i][1];
        out[4 * i + 2] = (float)r[i][2];
        out[4 * i + 3] = (float)(-((r[i][0] * t0 + r[i][1] * t1) + r[i][2] * t2));
    }
}

// The frame of workgroup (blockIdx.x, blockIdx.y): view index, its environment, the pixel and workgroup offsets of its
// camera inside the environment.  -> false where the workgroup lies beyond its frame (frames differ in size).
struct PcFrame {
    int view, e, pix_off, blk_off, npix;
};

__device__ __forceinline__ bool pc_frame(const PcArgs &a, PcFrame &f) {
    f.view = (int)blockIdx.y;
    f.e = f.view / a.C;
    const int c = f.view - f.e * a.C;
    f.pix_off = 0;
    f.blk_off = 0;
    for (int k = 0; k < c; k++) {
        const int n = a.v[f.e * a.C + k].W * a.v[f.e * a.C + k].H;
        f.pix_off += n;
        f.blk_off += (n + kPcBlock - 1) / kPcBlock;
    }
    f.npix = a.v[f.view].W * a.v[f.view].H;
    return (int)blockIdx.x * kPcBlock < f.npix;
}

struct PcPoint {
    float q[3];
    int16_t label;
    uint32_t rgb;  // r | g << 8 | b << 16
    bool ok;
};

// The definition above for pixel `pix` of view v (m: its C2W, rows of 4).
__device__ __forceinline__ PcPoint pc_point(const PcArgs &a, const PcView &v, const float *m, int pix) {
    PcPoint pt;
    pt.ok = false;
    pt.q[0] = pt.q[1] = pt.q[2] = 0.0f;
    pt.label = -1;
    pt.rgb = 0u;
    if (pix >= v.W * v.H) return pt;
    const float d = v.depth[pix];
    if (!(d > 0.0f)) return pt;
    const int y = pix / v.W, x = pix - y * v.W;
    const float z = d / v.depth_scale;
    const float ndx = (float)(2 * x + 1) / (float)v.W - 1.0f, ndy = (float)(2 * y + 1) / (float)v.H - 1.0f;
    const float xv = (ndx * v.tanfovx) * z, yv = (ndy * v.tanfovy) * z, zv = z;
    float p[3];
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = ((m[4 * i] * xv + m[4 * i + 1] * yv) + m[4 * i + 2] * zv) + m[4 * i + 3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        pt.q[i] = ((a.A[4 * i] * p[0] + a.A[4 * i + 1] * p[1]) + a.A[4 * i + 2] * p[2]) + a.A[4 * i + 3];
        if (a.crop) ok = ok && pt.q[i] >= a.lo[i] && pt.q[i] <= a.hi[i];
    }
    if (v.label != nullptr) pt.label = v.label[pix];
    if (a.excl != nullptr) {
        const uint32_t u = (uint32_t)(uint16_t)pt.label;
        ok = ok && ((a.excl[u >> 5] >> (u & 31u)) & 1u) == 0u;
    }
    if (v.rgb != nullptr) {
        const uint8_t *c = v.rgb + 3 * (size_t)pix;
        pt.rgb = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
    }
    pt.ok = ok;
    return pt;
}

__device__ __forceinline__ void pc_write(const PcArgs &a, size_t slot, bool ok, const float *q, uint32_t rgb, int16_t label) {
    a.xyzw[slot] = ok ? make_float4(q[0], q[1], q[2], 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint8_t *c = a.rgb + 3 * slot;
    c[0] = ok ? (uint8_t)(rgb & 255u) : (uint8_t)0;
    c[1] = ok ? (uint8_t)((rgb >> 8) & 255u) : (uint8_t)0;
    c[2] = ok ? (uint8_t)((rgb >> 16) & 255u) : (uint8_t)0;
    a.seg[slot] = ok ? label : (int16_t)-1;
}

// The frame's C2W into LDS (thread 0, binary64), shared after the barrier.
__device__ __forceinline__ void pc_load_c2w(const PcView &v, float *s_m) {
    if (threadIdx.x == 0) pc_c2w(v.vm, s_m);
    __syncthreads();
}

__global__ __launch_bounds__(kPcBlock) void pc_pixel_kernel(const PcArgs a) {
    __shared__ float s_m[12];
    __shared__ int s_cnt[kPcBlock / GSR_WAVE];
    PcFrame f;
    if (!pc_frame(a, f)) return;  // (uniform over the workgroup)
    const PcView &v = a.v[f.view];
    pc_load_c2w(v, s_m);
    const int pix = (int)blockIdx.x * kPcBlock + (int)threadIdx.x;
    const PcPoint pt = pc_point(a, v, s_m, pix);
    if (a.mode == GSR_PC_DENSE && pix < f.npix)
        pc_write(a, (size_t)f.e * a.N + f.pix_off + pix, pt.ok, pt.q, pt.rgb, pt.label);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(pt.ok);
    if (gsr_lane() == 0) s_cnt[gsr_wave()] = (int)__builtin_popcountll(mask);
    __syncthreads();
    if (threadIdx.x == 0) a.blk[(size_t)f.e * a.NB + f.blk_off + blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__device__ __forceinline__ int pc_selected(const PcArgs &a, int n) {
    const int cap = a.mode == GSR_PC_STRIDE ? a.K : a.Mcap;
    return n < cap ? n : cap;
}

__global__ __launch_bounds__(1024) void pc_scan_kernel(const PcArgs a) {
    __shared__ uint32_t s_w[1024 / GSR_WAVE];
    const int e = (int)blockIdx.x;
    int32_t *blk = a.blk + (size_t)e * a.NB;
    uint32_t carry = 0;
    for (int base = 0; base < a.NB; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const uint32_t v = i < a.NB ? (uint32_t)blk[i] : 0u;
        const uint32_t incl = gsr_wave_incl_scan(v);
        if (gsr_lane() == 63) s_w[gsr_wave()] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < 1024 / GSR_WAVE; w++) {
            const uint32_t t = s_w[w];
            if (w < gsr_wave()) before += t;
            total += t;
        }
        if (i < a.NB) blk[i] = (int32_t)(carry + before + incl - v);
        carry += total;
        __syncthreads();  // (s_w is rewritten by the next chunk)
    }
    const int n = (int)carry;
    int cnt = n;
    if (a.mode != GSR_PC_DENSE) {
        cnt = pc_selected(a, n);
        if (a.mode == GSR_PC_FPS && cnt > a.K) cnt = a.K;
    }
    if (threadIdx.x == 0) {
        a.env_n[e] = n;
        a.count[e] = cnt;
    }
    if (a.mode == GSR_PC_STRIDE) {
        const float q0[3] = {0.0f, 0.0f, 0.0f};
        for (int j = cnt + (int)threadIdx.x; j < a.K; j += 1024) pc_write(a, (size_t)e * a.K + j, false, q0, 0u, -1);
    }
}

__global__ __launch_bounds__(kPcBlock) void pc_select_kernel(const PcArgs a) {
    __shared__ float s_m[12];
    __shared__ int s_cnt[kPcBlock / GSR_WAVE];
    PcFrame f;
    if (!pc_frame(a, f)) return;
    const PcView &v = a.v[f.view];
    pc_load_c2w(v, s_m);
    const int pix = (int)blockIdx.x * kPcBlock + (int)threadIdx.x;
    const PcPoint pt = pc_point(a, v, s_m, pix);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(pt.ok);
    const int lane_rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (gsr_lane() == 0) s_cnt[gsr_wave()] = (int)__builtin_popcountll(mask);
    __syncthreads();
    if (!pt.ok) return;
    int r = a.blk[(size_t)f.e * a.NB + f.blk_off + blockIdx.x] + lane_rank;
    for (int w = 0; w < gsr_wave(); w++) r += s_cnt[w];
    const int n = a.env_n[f.e];
    const int M = pc_selected(a, n);
    const int64_t j = ((int64_t)r * M + n - 1) / n;  // (n > 0: this point is valid)
    if (j >= M || (j * n) / M != (int64_t)r) return;
    if (a.mode == GSR_PC_STRIDE) {
        pc_write(a, (size_t)f.e * a.K + (size_t)j, true, pt.q, pt.rgb, pt.label);
    } else {
        const size_t s = (size_t)f.e * a.Mcap + (size_t)j;
        a.cand[s] = make_float4(pt.q[0], pt.q[1], pt.q[2], __uint_as_float(pt.rgb));
        a.cand_seg[s] = pt.label;
    }
}

// max of 64-bit keys over the wave, in DPP moves (the pattern of gsr_wave_incl_scan; 0 is the identity): lane 63 holds it
__device__ __forceinline__ uint64_t pc_wave_max_u64(uint64_t k) {
    uint32_t lo = (uint32_t)k, hi = (uint32_t)(k >> 32);
#define PC_DPP_MAX(ctrl, rmask, bound)                                                                                     \
    {                                                                                                                  \
        const uint32_t ol = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, ctrl, rmask, 0xf, bound);               \
        const uint32_t oh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, ctrl, rmask, 0xf, bound);               \
        const uint64_t o = ((uint64_t)oh << 32) | ol, m = ((uint64_t)hi << 32) | lo;                                  \
        if (o > m) {                                                                                                   \
            lo = ol;                                                                                                   \
            hi = oh;                                                                                                   \
        }                                                                                                              \
    }
    PC_DPP_MAX(0x111, 0xf, true)   // row_shr:1
    PC_DPP_MAX(0x112, 0xf, true)   // row_shr:2
    PC_DPP_MAX(0x114, 0xf, true)   // row_shr:4
    PC_DPP_MAX(0x118, 0xf, true)   // row_shr:8
    PC_DPP_MAX(0x142, 0xa, false)  // row_bcast:15 -> rows 1, 3
    PC_DPP_MAX(0x143, 0xc, false)  // row_bcast:31 -> rows 2, 3
#undef PC_DPP_MAX
    const uint32_t l63 = (uint32_t)__builtin_amdgcn_readlane((int)lo, 63), h63 = (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);
    return ((uint64_t)h63 << 32) | l63;
}

template <int PER>
__global__ __launch_bounds__(kFpsThreads) void pc_fps_kernel(const PcArgs a) {
    __shared__ uint64_t s_key[2][kFpsWaves];
    __shared__ float4 s_sel[2][kFpsWaves];
    __shared__ int32_t s_pick[GSR_PC_MAX_K];
    const int e = (int)blockIdx.x, t = (int)threadIdx.x, lane = gsr_lane(), wave = gsr_wave();
    const int n = a.env_n[e];
    const int M = n < a.Mcap ? n : a.Mcap;
    const int picks = M < a.K ? M : a.K;
    const float4 *cand = a.cand + (size_t)e * a.Mcap;
    float px[PER], py[PER], pz[PER], dmin[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = t + k * kFpsThreads;
        px[k] = py[k] = pz[k] = 0.0f;
        dmin[k] = -1.0f;  // (no candidate: never above a best that starts at -1)
        if (i < M) {
            const float4 c = cand[i];
            px[k] = c.x;
            py[k] = c.y;
            pz[k] = c.z;
            dmin[k] = INFINITY;
        }
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (picks > 0) {
        const float4 c0 = cand[0];
        sx = c0.x;
        sy = c0.y;
        sz = c0.z;
        if (t == 0) s_pick[0] = 0;
    }
    int buf = 0;
    for (int it = 1; it < picks; it++) {
        float best = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
        int bk = -1;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const float dx = px[k] - sx, dy = py[k] - sy, dz = pz[k] - sz;
            const float d = ((dx * dx) + (dy * dy)) + dz * dz;
            dmin[k] = d < dmin[k] ? d : dmin[k];
            const bool better = dmin[k] > best;  // (strict: of equal values the lower index, k ascending, stays)
            best = better ? dmin[k] : best;
            bk = better ? k : bk;
            bx = better ? px[k] : bx;
            by = better ? py[k] : by;
            bz = better ? pz[k] : bz;
        }
        const uint64_t key = bk >= 0 ? (((uint64_t)__float_as_uint(best) << 32) | (uint64_t)(~(uint32_t)(t + bk * kFpsThreads)))
                                     : 0ull;
        const uint64_t wmax = pc_wave_max_u64(key);
        if (key == wmax && wmax != 0ull) {  // (the wave's winner: indices are unique, so is its key)
            s_key[buf][wave] = wmax;
            s_sel[buf][wave] = make_float4(bx, by, bz, 0.0f);
        } else if (lane == 63 && wmax == 0ull) {
            s_key[buf][wave] = 0ull;
        }
        __syncthreads();
        // (the 16 wave maxima as a tree, four compares deep: the keys are unique, so any order finds the same one)
        uint64_t kk[kFpsWaves];
        int kw[kFpsWaves];
#pragma unroll
        for (int w = 0; w < kFpsWaves; w++) {
            kk[w] = s_key[buf][w];
            kw[w] = w;
        }
#pragma unroll
        for (int h = kFpsWaves / 2; h >= 1; h >>= 1) {
#pragma unroll
            for (int w = 0; w < h; w++) {
                const bool up = kk[w + h] > kk[w];
                kk[w] = up ? kk[w + h] : kk[w];
                kw[w] = up ? kw[w + h] : kw[w];
            }
        }
        const uint64_t top = kk[0];
        const int tw = kw[0];
        const float4 s = s_sel[buf][tw];
        sx = s.x;
        sy = s.y;
        sz = s.z;
        if (t == 0) s_pick[it] = (int32_t)(~(uint32_t)top);
        buf ^= 1;  // (this iteration's slots are read before the next barrier, rewritten only after it)
    }
    __syncthreads();
    const int16_t *cseg = a.cand_seg + (size_t)e * a.Mcap;
    for (int j = t; j < a.K; j += kFpsThreads) {
        const size_t slot = (size_t)e * a.K + j;
        if (j < picks) {
            const int i = s_pick[j];
            const float4 c = cand[i];
            const float q[3] = {c.x, c.y, c.z};
            pc_write(a, slot, true, q, __float_as_uint(c.w), cseg[i]);
        } else {
            const float q0[3] = {0.0f, 0.0f, 0.0f};
            pc_write(a, slot, false, q0, 0u, -1);
        }
    }
}

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct PcLayout {
    int NB, N, max_blocks;
    int64_t blk, env_n, cand, cand_seg, bytes;
};

int pc_check(const GsrCloudSpec *s, PcLayout &L, bool need_buffers) {
    if (!s) {
        gsr_set_error("gsr_render_pointcloud: null spec");
        return GSR_E_INVALID;
    }
    if (s->struct_size != (int32_t)sizeof(GsrCloudSpec)) {
        gsr_set_error("gsr_render_pointcloud: struct_size %d, this library's GsrCloudSpec has %d bytes", (int)s->struct_size,
                      (int)sizeof(GsrCloudSpec));
        return GSR_E_INVALID;
    }
    if (s->E < 1 || s->C < 1 || s->E * s->C > GSR_PC_MAX_VIEWS || !s->views) {
        gsr_set_error("gsr_render_pointcloud: need 1 <= E, 1 <= C, E*C <= %d and a view array", GSR_PC_MAX_VIEWS);
        return GSR_E_INVALID;
    }
    if (s->mode < GSR_PC_DENSE || s->mode > GSR_PC_FPS) {
        gsr_set_error("gsr_render_pointcloud: unknown mode %d", (int)s->mode);
        return GSR_E_INVALID;
    }
    if (s->mode != GSR_PC_DENSE && (s->K < 1 || s->K > GSR_PC_MAX_K)) {
        gsr_set_error("gsr_render_pointcloud: K must be in [1, %d]", GSR_PC_MAX_K);
        return GSR_E_INVALID;
    }
    if (s->mode == GSR_PC_FPS && (s->fps_candidates < 1 || s->fps_candidates > GSR_PC_MAX_FPS_CANDIDATES)) {
        gsr_set_error("gsr_render_pointcloud: fps_candidates must be in [1, %d]", GSR_PC_MAX_FPS_CANDIDATES);
        return GSR_E_INVALID;
    }
    L.NB = 0;
    L.N = 0;
    L.max_blocks = 0;
    for (int c = 0; c < s->C; c++) {
        for (int e = 0; e < s->E; e++) {
            const GsrCloudView &v = s->views[e * s->C + c];
            const GsrCloudView &v0 = s->views[c];
            if (v.width < 1 || v.height < 1 || (int64_t)v.width * v.height > GSR_PC_MAX_VIEW_PIXELS ||
                v.width != v0.width || v.height != v0.height) {
                gsr_set_error("gsr_render_pointcloud: view (%d, %d): empty, larger than %d pixels, or a size other than "
                              "environment 0's camera %d", e, c, GSR_PC_MAX_VIEW_PIXELS, c);
                return GSR_E_INVALID;
            }
            if (need_buffers && (!v.viewmatrix || !v.depth)) {
                gsr_set_error("gsr_render_pointcloud: view (%d, %d): null view matrix or depth", e, c);
                return GSR_E_INVALID;
            }
            if (need_buffers && s->exclude && !v.label) {
                gsr_set_error("gsr_render_pointcloud: view (%d, %d): an exclusion set needs label maps", e, c);
                return GSR_E_INVALID;
            }
            if (need_buffers && !(v.depth_scale != 0.0f)) {
                gsr_set_error("gsr_render_pointcloud: view (%d, %d): depth_scale must be non-zero", e, c);
                return GSR_E_INVALID;
            }
        }
        const int n = s->views[c].width * s->views[c].height, nb = (n + kPcBlock - 1) / kPcBlock;
        if ((int64_t)L.N + n > (int64_t)GSR_PC_MAX_VIEW_PIXELS * 4) {
            gsr_set_error("gsr_render_pointcloud: more than %d pixels per environment", GSR_PC_MAX_VIEW_PIXELS * 4);
            return GSR_E_INVALID;
        }
        L.N += n;
        L.NB += nb;
        L.max_blocks = nb > L.max_blocks ? nb : L.max_blocks;
    }
    const int64_t E = s->E, Mcap = s->mode == GSR_PC_FPS ? s->fps_candidates : 0;
    L.blk = 0;
    L.env_n = align256(L.blk + E * L.NB * 4);
    L.cand = align256(L.env_n + E * 4);
    L.cand_seg = align256(L.cand + E * Mcap * 16);
    L.bytes = align256(L.cand_seg + E * Mcap * 2);
    return GSR_OK;
}

}  // namespace

extern "C" int gsr_pointcloud_workspace(const GsrCloudSpec *spec, int64_t *bytes) {
    PcLayout L;
    if (!bytes) {
        gsr_set_error("gsr_pointcloud_workspace: null bytes");
        return GSR_E_INVALID;
    }
    if (int r = pc_check(spec, L, false)) return r;
    *bytes = L.bytes;
    return GSR_OK;
}

extern "C" int gsr_render_pointcloud(const GsrCloudSpec *s, void *stream_) {
    PcLayout L;
    if (int r = pc_check(s, L, true)) return r;
    if (!s->out_xyzw || !s->out_rgb || !s->out_segmentation || !s->out_count) {
        gsr_set_error("gsr_render_pointcloud: the four outputs are required");
        return GSR_E_INVALID;
    }
    if (!s->workspace || s->workspace_bytes < L.bytes) {
        gsr_set_error("gsr_render_pointcloud: workspace of %lld bytes needed (gsr_pointcloud_workspace)", (long long)L.bytes);
        return GSR_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    PcArgs a;
    memset(&a, 0, sizeof(a));  // (nothing uninitialised travels in the kernarg)
    for (int k = 0; k < s->E * s->C; k++) {
        const GsrCloudView &v = s->views[k];
        a.v[k].vm = v.viewmatrix;
        a.v[k].depth = v.depth;
        a.v[k].label = v.label;
        a.v[k].rgb = v.rgb8;
        a.v[k].W = v.width;
        a.v[k].H = v.height;
        a.v[k].tanfovx = v.tanfovx;
        a.v[k].tanfovy = v.tanfovy;
        a.v[k].depth_scale = v.depth_scale;
    }
    memcpy(a.A, s->out_from_scene, sizeof(a.A));
    for (int i = 0; i < 3; i++) {
        a.lo[i] = s->crop_lo[i];
        a.hi[i] = s->crop_hi[i];
    }
    a.crop = s->crop ? 1 : 0;
    a.excl = s->exclude;
    a.xyzw = reinterpret_cast<float4 *>(s->out_xyzw);
    a.rgb = s->out_rgb;
    a.seg = s->out_segmentation;
    a.count = s->out_count;
    char *ws = (char *)s->workspace;
    a.blk = (int32_t *)(ws + L.blk);
    a.env_n = (int32_t *)(ws + L.env_n);
    a.cand = (float4 *)(ws + L.cand);
    a.cand_seg = (int16_t *)(ws + L.cand_seg);
    a.E = s->E;
    a.C = s->C;
    a.NB = L.NB;
    a.N = L.N;
    a.mode = s->mode;
    a.K = s->mode == GSR_PC_DENSE ? 0 : s->K;
    a.Mcap = s->mode == GSR_PC_FPS ? s->fps_candidates : 0;
    const bool debug = false;
    hipLaunchKernelGGL(pc_pixel_kernel, dim3(L.max_blocks, s->E * s->C), dim3(kPcBlock), 0, stream, a);
    if (int r = gsr_check_launch("pointcloud pixel pass", debug, stream)) return r;
    hipLaunchKernelGGL(pc_scan_kernel, dim3(s->E), dim3(1024), 0, stream, a);
    if (int r = gsr_check_launch("pointcloud scan", debug, stream)) return r;
    if (s->mode == GSR_PC_DENSE) return GSR_OK;
    hipLaunchKernelGGL(pc_select_kernel, dim3(L.max_blocks, s->E * s->C), dim3(kPcBlock), 0, stream, a);
    if (int r = gsr_check_launch("pointcloud select", debug, stream)) return r;
    if (s->mode == GSR_PC_STRIDE) return GSR_OK;
    if (a.Mcap <= 8 * kFpsThreads)
        hipLaunchKernelGGL(pc_fps_kernel<8>, dim3(s->E), dim3(kFpsThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(pc_fps_kernel<16>, dim3(s->E), dim3(kFpsThreads), 0, stream, a);
    return gsr_check_launch("pointcloud fps", debug, stream);
}
