// nnquery.hip -- nearest point of a reference cloud for every point of a query cloud, exact, and the two real2sim steps
// on top of it: label transfer with bounding-box validation and the sums of one scaled point-to-point ICP update
// (include/gsr.h holds the definitions; GSWorld real2sim_utils/segment_utils.py and real2sim/scripts/icp.py are the users).
//
// The search is knn.hip's plan cut for two clouds.  The reference cloud is put in Morton order once (gsr_nn_build), in
// boxes of 1024 consecutive points with AABBs.  A query call sorts the queries by their Morton code IN THE REFERENCE'S
// GRID (codes clamp to its faces: far-away queries gather at the ends), so that the 64 queries of a wave are neighbours
// in space; the wave decides per box for all its lanes at once and streams a wanted box through registers with
// readlane broadcasts.  Every candidate is a (d2, caller's index) pair packed into one 64-bit key -- d2 >= +0, so its bits
// order as an integer -- and a query keeps the minimum key: the lowest index wins a tie without a branch, and the result
// is the O(n m) definition whatever order the candidates arrive in.  A box is skipped only when its lower bound is strictly
// above the query's current d2 (an equal bound may hide a tie with a lower index); a distance limit starts the key at
// (max_dist2, no index), which prunes everything beyond it from the first box on.
#include "morton_boxes.h"

namespace {

constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

struct NnIndex {
    float *minmax;          // [6] min xyz, max xyz of the cloud: the grid of the codes
    uint32_t *n_dev;        // [1]
    uint32_t *key[2];       // [n] key[0]: the sorted codes
    uint32_t *idx[2];       // [n] idx[0]: sorted position -> caller's number
    uint32_t *rank;         // [n] caller's number -> sorted position
    float *sorted_pts;      // [3n]
    float *boxes;           // [nbox][6]
    float *minmax_partial;  // [256][6]   (from here on: scratch of the build)
    uint32_t *sort_table;
    uint32_t *sort_totals;
    static NnIndex carve(char *base, int32_t n_ref, size_t *bytes = nullptr) {
        NnIndex s;
        char *p = base;
        const size_t n = (size_t)(n_ref > 0 ? n_ref : 1);
        s.minmax = GeomState::take<float>(p, 8);
        s.n_dev = GeomState::take<uint32_t>(p, 1);
        s.key[0] = GeomState::take<uint32_t>(p, n);
        s.idx[0] = GeomState::take<uint32_t>(p, n);
        s.rank = GeomState::take<uint32_t>(p, n);
        s.sorted_pts = GeomState::take<float>(p, 3 * n);
        s.boxes = GeomState::take<float>(p, 6 * (size_t)gsr_div_up(n, kBox));
        s.key[1] = GeomState::take<uint32_t>(p, n);
        s.idx[1] = GeomState::take<uint32_t>(p, n);
        s.minmax_partial = GeomState::take<float>(p, 256 * 6);
        s.sort_table = GeomState::take<uint32_t>(p, (size_t)GSR_DEPTH_RADIX_BINS * GeomState::sort_blocks(n_ref));
        s.sort_totals = GeomState::take<uint32_t>(p, GSR_DEPTH_RADIX_BINS);
        if (bytes) *bytes = (size_t)(p - base);
        return s;
    }
};

struct NnQueryWs {
    uint32_t *n_dev;        // [1]
    uint32_t *key[2];       // [m]
    uint32_t *idx[2];       // [m] idx[0]: sorted position -> query number
    float *tq;              // [3m] the transformed queries
    uint32_t *sort_table;
    uint32_t *sort_totals;
    static NnQueryWs carve(char *base, int32_t n_query, size_t *bytes = nullptr) {
        NnQueryWs s;
        char *p = base;
        const size_t m = (size_t)(n_query > 0 ? n_query : 1);
        s.n_dev = GeomState::take<uint32_t>(p, 1);
        s.key[0] = GeomState::take<uint32_t>(p, m);
        s.key[1] = GeomState::take<uint32_t>(p, m);
        s.idx[0] = GeomState::take<uint32_t>(p, m);
        s.idx[1] = GeomState::take<uint32_t>(p, m);
        s.tq = GeomState::take<float>(p, 3 * m);
        s.sort_table = GeomState::take<uint32_t>(p, (size_t)GSR_DEPTH_RADIX_BINS * GeomState::sort_blocks(n_query));
        s.sort_totals = GeomState::take<uint32_t>(p, GSR_DEPTH_RADIX_BINS);
        if (bytes) *bytes = (size_t)(p - base);
        return s;
    }
};

struct Xform {
    float m[12];
};

__device__ __forceinline__ void apply_xform(const Xform &M, int use, float x, float y, float z, float (&o)[3]) {
    o[0] = x;
    o[1] = y;
    o[2] = z;
    if (use) {
#pragma unroll
        for (int r = 0; r < 3; r++) o[r] = fma_(M.m[4 * r + 2], z, fma_(M.m[4 * r + 1], y, M.m[4 * r] * x)) + M.m[4 * r + 3];
    }
}

__global__ __launch_bounds__(GSR_BLOCK) void nn_rank_kernel(int n, const uint32_t *__restrict__ order,
                                                            uint32_t *__restrict__ rank) {
    const int s = blockIdx.x * GSR_BLOCK + (int)threadIdx.x;
    if (s < n) rank[order[s]] = (uint32_t)s;
}

// transformed queries, their codes in the reference's grid (minmax == nullptr: an empty reference, every code 0)
__global__ __launch_bounds__(GSR_BLOCK) void nn_query_code_kernel(int m, const float *__restrict__ query, Xform M, int use,
                                                                  const float *__restrict__ minmax, float *__restrict__ tq,
                                                                  float *__restrict__ query_out, uint32_t *__restrict__ keys,
                                                                  uint32_t *__restrict__ idx, uint32_t *__restrict__ n_dev) {
    const int i = blockIdx.x * GSR_BLOCK + (int)threadIdx.x;
    if (i == 0) *n_dev = (uint32_t)m;
    if (i >= m) return;
    float v[3];
    apply_xform(M, use, query[3 * (size_t)i], query[3 * (size_t)i + 1], query[3 * (size_t)i + 2], v);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        tq[3 * (size_t)i + c] = v[c];
        if (query_out != nullptr) query_out[3 * (size_t)i + c] = v[c];
    }
    keys[i] = minmax != nullptr ? morton_code(v, minmax) : 0u;  // (a NaN coordinate clamps to cell 0: any place will do)
    idx[i] = (uint32_t)i;
}

__device__ __forceinline__ uint64_t cand_key(float d, uint32_t index) {
    return ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)index;
}

__global__ __launch_bounds__(GSR_BLOCK) void nn_search_kernel(int m, const float *__restrict__ tq,
                                                              const uint32_t *__restrict__ qorder,
                                                              const uint32_t *__restrict__ qkeys, int n,
                                                              const float *__restrict__ sp,
                                                              const uint32_t *__restrict__ keys,
                                                              const uint32_t *__restrict__ order,
                                                              const float *__restrict__ boxes, int nbox, float max_dist2,
                                                              int32_t *__restrict__ out_index, float *__restrict__ out_dist2) {
    const int s = blockIdx.x * GSR_BLOCK + (int)threadIdx.x;  // sorted position of the query
    const bool valid = s < m;
    const int sc = valid ? s : m - 1;
    const uint32_t q = qorder[sc];
    float px = tq[3 * (size_t)q], py = tq[3 * (size_t)q + 1], pz = tq[3 * (size_t)q + 2];
    const bool finite = fabsf(px) <= FLT_MAX && fabsf(py) <= FLT_MAX && fabsf(pz) <= FLT_MAX;  // false on NaN
    if (!finite) px = py = pz = 0.f;
    const bool active = valid && finite;
    uint64_t best = cand_key(max_dist2 >= 0.f ? max_dist2 : __builtin_inff(), kNoIndex);
    if (n > 0) {
        // seed: the +-3 neighbours of the query's code in the sorted reference codes (real candidates, index and all)
        const uint32_t code = qkeys[sc];
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < code) lo = mid + 1; else hi = mid;
        }
        for (int o = -3; o <= 3; o++) {
            const int t = lo + o;
            if (t < 0 || t >= n) continue;
            const uint64_t k = cand_key(dist2(px, py, pz, sp[3 * (size_t)t], sp[3 * (size_t)t + 1], sp[3 * (size_t)t + 2]),
                                        order[t]);
            best = k < best ? k : best;
        }
    }
    const int lane = gsr_lane();
    for (int b = 0; b < nbox; b++) {
        const float dbox = box_dist2(px, py, pz, boxes + 6 * (size_t)b);
        const bool want = active && !(dbox > __uint_as_float((uint32_t)(best >> 32)));
        if (__ballot(want) == 0ull) continue;  // wave-uniform: nobody needs this box
        const int start = b * kBox;
        const int end = min(n, start + kBox);
        for (int base = start; base < end; base += 64) {
            const int t = base + lane;
            const int tc = t < end ? t : end - 1;
            const float qx = sp[3 * (size_t)tc], qy = sp[3 * (size_t)tc + 1], qz = sp[3 * (size_t)tc + 2];
            const int oi = (int)order[tc];
            // (lanes past the box's end hold its last point once more: the same key again changes nothing, so every
            //  chunk is a fixed 64 candidates and the loop unrolls with constant lane selects)
#pragma unroll 16
            for (int j = 0; j < 64; j++) {
                const uint64_t k = cand_key(dist2(px, py, pz, bcast(qx, j), bcast(qy, j), bcast(qz, j)),
                                            (uint32_t)__builtin_amdgcn_readlane(oi, j));
                best = k < best ? k : best;
            }
        }
    }
    if (valid) {
        const bool found = active && (uint32_t)best != kNoIndex;
        out_index[q] = found ? (int32_t)(uint32_t)best : -1;
        out_dist2[q] = found ? __uint_as_float((uint32_t)(best >> 32)) : __builtin_inff();
    }
}

// ---- label transfer ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float label_box_dist2(float px, float py, float pz, const float *bx) {
    const float ex = fmaxf(fmaxf(bx[0] - px, 0.f), px - bx[3]);
    const float ey = fmaxf(fmaxf(bx[1] - py, 0.f), py - bx[4]);
    const float ez = fmaxf(fmaxf(bx[2] - pz, 0.f), pz - bx[5]);
    return fma_(ez, ez, fma_(ey, ey, ex * ex));
}

__global__ __launch_bounds__(GSR_BLOCK) void label_transfer_kernel(int n, const int32_t *__restrict__ index,
                                                                   const float *__restrict__ pts,
                                                                   const int32_t *__restrict__ ref_labels, int n_ref,
                                                                   int n_boxes, const int32_t *__restrict__ box_labels,
                                                                   const float *__restrict__ box_bounds, float thr2,
                                                                   int32_t *__restrict__ labels) {
    extern __shared__ float s_mem[];  // [6 n_boxes] bounds, then [n_boxes] labels
    float *s_box = s_mem;
    int32_t *s_lab = reinterpret_cast<int32_t *>(s_mem + 6 * (size_t)n_boxes);
    for (int k = (int)threadIdx.x; k < 6 * n_boxes; k += GSR_BLOCK) s_box[k] = box_bounds[k];
    for (int k = (int)threadIdx.x; k < n_boxes; k += GSR_BLOCK) s_lab[k] = box_labels[k];
    __syncthreads();
    const int i = blockIdx.x * GSR_BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const int32_t j = index[i];
    int32_t L = (j >= 0 && j < n_ref) ? ref_labels[j] : -1;
    if (L != -1) {
        const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
        int row = -1;
        for (int k = 0; k < n_boxes; k++)
            if (s_lab[k] == L) { row = k; break; }
        if (row < 0) {
            L = -1;
        } else if (label_box_dist2(px, py, pz, s_box + 6 * row) > thr2) {
            float bestd = __builtin_inff();
            L = -1;
            for (int k = 0; k < n_boxes; k++) {
                const float d = label_box_dist2(px, py, pz, s_box + 6 * k);
                if (d < bestd && d <= thr2) {
                    bestd = d;
                    L = s_lab[k];
                }
            }
        }
    }
    labels[i] = L;
}

// ---- ICP moments ---------------------------------------------------------------------------------------------------------
constexpr int kMoments = 18;
constexpr int kMomentBlocks = 256;
static_assert(kMomentBlocks * kMoments * sizeof(double) == GSR_ICP_WORKSPACE_BYTES, "include/gsr.h states the workspace size");

__global__ __launch_bounds__(GSR_BLOCK) void icp_moments_partial_kernel(int n, const float *__restrict__ src, Xform M, int use,
                                                                        int n_ref, const float *__restrict__ sp,
                                                                        const uint32_t *__restrict__ rank,
                                                                        const int32_t *__restrict__ index,
                                                                        const float *__restrict__ d2,
                                                                        double *__restrict__ partial) {
    __shared__ double s_red[4][kMoments];
    double a[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; k++) a[k] = 0.0;
    for (int i = blockIdx.x * GSR_BLOCK + (int)threadIdx.x; i < n; i += gridDim.x * GSR_BLOCK) {
        const int32_t j = index[i];
        if (j < 0 || j >= n_ref) continue;
        float pf[3];
        apply_xform(M, use, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], pf);
        const uint32_t r = rank[j];
        const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        const double q[3] = {(double)sp[3 * (size_t)r], (double)sp[3 * (size_t)r + 1], (double)sp[3 * (size_t)r + 2]};
        a[0] += 1.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a[1 + c] += p[c];
            a[4 + c] += q[c];
#pragma unroll
            for (int e = 0; e < 3; e++) a[7 + 3 * c + e] += p[c] * q[e];
        }
        a[16] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        a[17] += (double)d2[i];
    }
#pragma unroll
    for (int k = 0; k < kMoments; k++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
    if (gsr_lane() == 0)
#pragma unroll
        for (int k = 0; k < kMoments; k++) s_red[gsr_wave()][k] = a[k];
    __syncthreads();
    if (threadIdx.x < kMoments) {
        const int k = (int)threadIdx.x;
        partial[blockIdx.x * kMoments + k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    }
}

__global__ void icp_moments_final_kernel(int nblocks, const double *__restrict__ partial, double *__restrict__ sums) {
    const int k = (int)threadIdx.x;
    if (k >= kMoments) return;
    double v = 0.0;
    for (int b = 0; b < nblocks; b++) v += partial[b * kMoments + k];
    sums[k] = v;
}

bool misaligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" size_t gsr_nn_index_bytes(int32_t n_ref) {
    size_t bytes = 0;
    NnIndex::carve(nullptr, n_ref, &bytes);
    return bytes;
}

extern "C" int gsr_nn_build(int32_t n_ref, const float *ref, void *index_mem, size_t index_bytes, void *stream_) {
    if (n_ref < 0 || (n_ref > 0 && (!ref || !index_mem))) {
        gsr_set_error("gsr_nn_build: null pointer or negative n_ref");
        return GSR_E_INVALID;
    }
    if (n_ref == 0) return GSR_OK;
    if (index_bytes < gsr_nn_index_bytes(n_ref) || misaligned(index_mem, 256)) {
        gsr_set_error("gsr_nn_build: index memory too small or not 256-byte aligned");
        return GSR_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const NnIndex s = NnIndex::carve((char *)index_mem, n_ref);
    const int nred = min(256, gsr_div_up(n_ref, GSR_BLOCK));
    hipLaunchKernelGGL(knn_minmax_partial_kernel, dim3(nred), dim3(GSR_BLOCK), 0, stream, n_ref, ref, s.minmax_partial);
    hipLaunchKernelGGL(knn_minmax_final_kernel, dim3(1), dim3(64), 0, stream, nred, s.minmax_partial, s.minmax, s.n_dev,
                       (uint32_t)n_ref);
    // 30-bit codes, 11 bits per pass = 3 passes: start in side 1 so that the sorted order ends in side 0
    const int start = gsr_radix_passes(30, GSR_DEPTH_RADIX_BITS) & 1;
    hipLaunchKernelGGL(knn_morton_kernel, dim3(gsr_div_up(n_ref, GSR_BLOCK)), dim3(GSR_BLOCK), 0, stream, n_ref, ref, s.minmax,
                       s.key[start], s.idx[start]);
    if (int e = gsr_check_launch("nn_morton", false, stream)) return e;
    uint32_t *key[2] = {s.key[0], s.key[1]};
    uint32_t *val[2] = {s.idx[0], s.idx[1]};
    if (int e = gsr_radix_sort_u32(key, val, s.n_dev, n_ref, 30, GSR_DEPTH_RADIX_BITS, start, s.sort_table, s.sort_totals,
                                   false, stream))
        return e;
    hipLaunchKernelGGL(knn_gather_box_kernel, dim3(gsr_div_up(n_ref, kBox)), dim3(GSR_BLOCK), 0, stream, n_ref, ref, s.idx[0],
                       s.sorted_pts, s.boxes);
    hipLaunchKernelGGL(nn_rank_kernel, dim3(gsr_div_up(n_ref, GSR_BLOCK)), dim3(GSR_BLOCK), 0, stream, n_ref, s.idx[0], s.rank);
    return gsr_check_launch("nn_build", false, stream);
}

extern "C" size_t gsr_nn_query_workspace_bytes(int32_t n_query) {
    size_t bytes = 0;
    NnQueryWs::carve(nullptr, n_query, &bytes);
    return bytes;
}

extern "C" int gsr_nn_query(const GsrNnQuery *a, void *stream_) {
    if (!a || a->struct_size != (int32_t)sizeof(GsrNnQuery)) {
        gsr_set_error("gsr_nn_query: null argument or struct_size mismatch");
        return GSR_E_INVALID;
    }
    if (a->n_ref < 0 || a->n_query < 0 || a->max_dist2 != a->max_dist2) {
        gsr_set_error("gsr_nn_query: negative size or NaN max_dist2");
        return GSR_E_INVALID;
    }
    if (a->n_query == 0) return GSR_OK;
    if (!a->query || !a->index || !a->dist2 || !a->workspace || (a->n_ref > 0 && !a->index_mem)) {
        gsr_set_error("gsr_nn_query: null pointer");
        return GSR_E_INVALID;
    }
    if (a->workspace_bytes < (int64_t)gsr_nn_query_workspace_bytes(a->n_query) || misaligned(a->workspace, 256) ||
        (a->n_ref > 0 && (a->index_bytes < (int64_t)gsr_nn_index_bytes(a->n_ref) || misaligned(a->index_mem, 256)))) {
        gsr_set_error("gsr_nn_query: workspace or index memory too small or not 256-byte aligned");
        return GSR_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int m = a->n_query, n = a->n_ref;
    const float max_dist2 = a->max_dist2 + 0.f;  // (-0 becomes +0, a limit of zero: as bits, -0 would sort above +inf)
    const NnQueryWs w = NnQueryWs::carve((char *)a->workspace, m);
    NnIndex s = {};
    if (n > 0) s = NnIndex::carve((char *)const_cast<void *>(a->index_mem), n);
    Xform M;
    for (int k = 0; k < 12; k++) M.m[k] = a->query_transform[k];
    // (an empty reference: nothing to sort by -- the queries stay in side 0 in their own order)
    const int start = n > 0 ? (gsr_radix_passes(30, GSR_DEPTH_RADIX_BITS) & 1) : 0;
    hipLaunchKernelGGL(nn_query_code_kernel, dim3(gsr_div_up(m, GSR_BLOCK)), dim3(GSR_BLOCK), 0, stream, m, a->query, M,
                       a->use_transform != 0, n > 0 ? s.minmax : nullptr, w.tq, a->query_out, w.key[start], w.idx[start],
                       w.n_dev);
    if (int e = gsr_check_launch("nn_query_code", false, stream)) return e;
    if (n > 0) {
        uint32_t *key[2] = {w.key[0], w.key[1]};
        uint32_t *val[2] = {w.idx[0], w.idx[1]};
        if (int e = gsr_radix_sort_u32(key, val, w.n_dev, m, 30, GSR_DEPTH_RADIX_BITS, start, w.sort_table, w.sort_totals,
                                       false, stream))
            return e;
    }
    hipLaunchKernelGGL(nn_search_kernel, dim3(gsr_div_up(m, GSR_BLOCK)), dim3(GSR_BLOCK), 0, stream, m, w.tq, w.idx[0],
                       w.key[0], n, s.sorted_pts, s.key[0], s.idx[0], s.boxes, n > 0 ? gsr_div_up(n, kBox) : 0, max_dist2,
                       a->index, a->dist2);
    return gsr_check_launch("nn_search", false, stream);
}

extern "C" int gsr_label_transfer(const GsrLabelTransfer *a, void *stream_) {
    if (!a || a->struct_size != (int32_t)sizeof(GsrLabelTransfer)) {
        gsr_set_error("gsr_label_transfer: null argument or struct_size mismatch");
        return GSR_E_INVALID;
    }
    if (a->n < 0 || a->n_ref < 0 || a->n_boxes < 0 || a->n_boxes > GSR_LABEL_MAX_BOXES) {
        gsr_set_error("gsr_label_transfer: negative size or more than %d boxes", GSR_LABEL_MAX_BOXES);
        return GSR_E_INVALID;
    }
    if (a->n == 0) return GSR_OK;
    if (!a->index || !a->points || !a->labels || (a->n_ref > 0 && !a->ref_labels) ||
        (a->n_boxes > 0 && (!a->box_labels || !a->box_bounds))) {
        gsr_set_error("gsr_label_transfer: null pointer");
        return GSR_E_INVALID;
    }
    const float thr2 = a->threshold * a->threshold;
    hipLaunchKernelGGL(label_transfer_kernel, dim3(gsr_div_up(a->n, GSR_BLOCK)), dim3(GSR_BLOCK),
                       (size_t)a->n_boxes * 7 * sizeof(float), (hipStream_t)stream_, a->n, a->index, a->points, a->ref_labels,
                       a->n_ref, a->n_boxes, a->box_labels, a->box_bounds, thr2, a->labels);
    return gsr_check_launch("label_transfer", false, (hipStream_t)stream_);
}

extern "C" int gsr_icp_moments(const GsrIcpMoments *a, void *stream_) {
    if (!a || a->struct_size != (int32_t)sizeof(GsrIcpMoments)) {
        gsr_set_error("gsr_icp_moments: null argument or struct_size mismatch");
        return GSR_E_INVALID;
    }
    if (a->n < 0 || a->n_ref < 0) {
        gsr_set_error("gsr_icp_moments: negative size");
        return GSR_E_INVALID;
    }
    const bool work = a->n > 0 && a->n_ref > 0;
    if (!a->sums || !a->workspace || (work && (!a->source || !a->index || !a->dist2 || !a->index_mem))) {
        gsr_set_error("gsr_icp_moments: null pointer");
        return GSR_E_INVALID;
    }
    if (a->workspace_bytes < (int64_t)GSR_ICP_WORKSPACE_BYTES || misaligned(a->workspace, 8) || misaligned(a->sums, 8) ||
        (work && (a->index_bytes < (int64_t)gsr_nn_index_bytes(a->n_ref) || misaligned(a->index_mem, 256)))) {
        gsr_set_error("gsr_icp_moments: workspace or index memory too small or misaligned");
        return GSR_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    double *partial = (double *)a->workspace;
    int nblocks = 0;
    if (work) {
        const NnIndex s = NnIndex::carve((char *)const_cast<void *>(a->index_mem), a->n_ref);
        Xform M;
        for (int k = 0; k < 12; k++) M.m[k] = a->transform[k];
        nblocks = min(kMomentBlocks, gsr_div_up(a->n, GSR_BLOCK));
        hipLaunchKernelGGL(icp_moments_partial_kernel, dim3(nblocks), dim3(GSR_BLOCK), 0, stream, a->n, a->source, M,
                           a->use_transform != 0, a->n_ref, s.sorted_pts, s.rank, a->index, a->dist2, partial);
    }
    hipLaunchKernelGGL(icp_moments_final_kernel, dim3(1), dim3(64), 0, stream, nblocks, partial, a->sums);
    return gsr_check_launch("icp_moments", false, stream);
}
