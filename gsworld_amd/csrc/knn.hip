// knn.hip -- simple_knn distCUDA2: mean squared distance to the 3 nearest other points, exact
// (upstream simple-knn/simple_knn.cu).
//
// Same plan as upstream -- Morton order, boxes of 1024 consecutive points with AABBs, prune boxes by a reject
// radius seeded from the +-3 Morton neighbours -- re-cut for wave64: a wave owns 64 consecutive sorted points
// (spatially close), takes the box decision for all of them at once (scan a box if ANY lane needs it; extra
// candidates are harmless because every other point is a valid candidate), and streams the box's points
// through registers 64 at a time with readlane broadcasts, so there is no divergence and no LDS traffic.
// The result is bit-identical to the O(N^2) definition: the squared distance uses one fixed fmaf chain and
// the 3-best insertion is order-independent.
#include "morton_boxes.h"

namespace {

struct KnnState {
    float *minmax_partial;  // [256][6]
    float *minmax;          // [6] min xyz, max xyz
    uint32_t *n_dev;        // [1]
    uint32_t *key[2];       // [P]
    uint32_t *idx[2];       // [P]
    uint32_t *sort_table;   // [256 * nb]
    uint32_t *sort_totals;  // [256]
    float *sorted_pts;      // [P*3] points in Morton order (SoA-free: xyz interleaved)
    float *boxes;           // [nbox][6]
    static KnnState carve(char *base, int32_t P, size_t *bytes = nullptr) {
        KnnState s;
        char *p = base;
        const size_t n = (size_t)(P > 0 ? P : 1);
        s.minmax_partial = GeomState::take<float>(p, 256 * 6);
        s.minmax = GeomState::take<float>(p, 8);
        s.n_dev = GeomState::take<uint32_t>(p, 1);
        s.key[0] = GeomState::take<uint32_t>(p, n);
        s.key[1] = GeomState::take<uint32_t>(p, n);
        s.idx[0] = GeomState::take<uint32_t>(p, n);
        s.idx[1] = GeomState::take<uint32_t>(p, n);
        s.sort_table = GeomState::take<uint32_t>(p, (size_t)GSR_DEPTH_RADIX_BINS * GeomState::sort_blocks(P));
        s.sort_totals = GeomState::take<uint32_t>(p, GSR_DEPTH_RADIX_BINS);
        s.sorted_pts = GeomState::take<float>(p, 3 * n);
        s.boxes = GeomState::take<float>(p, 6 * (size_t)gsr_div_up(n, kBox));
        if (bytes) *bytes = (size_t)(p - base);
        return s;
    }
};

__device__ __forceinline__ void insert3(float &b0, float &b1, float &b2, float d) {
    if (b0 > d) { const float t = b0; b0 = d; d = t; }
    if (b1 > d) { const float t = b1; b1 = d; d = t; }
    if (b2 > d) { b2 = d; }
}

__global__ __launch_bounds__(GSR_BLOCK) void knn_search_kernel(int P, const float *__restrict__ sp,
                                                               const uint32_t *__restrict__ order,
                                                               const float *__restrict__ boxes, int nbox,
                                                               float *__restrict__ out) {
    const int s = blockIdx.x * GSR_BLOCK + (int)threadIdx.x;  // sorted position
    const bool valid = s < P;
    const int sc = valid ? s : P - 1;
    const float px = sp[3 * (size_t)sc], py = sp[3 * (size_t)sc + 1], pz = sp[3 * (size_t)sc + 2];
    // reject radius: third-best among the +-3 Morton neighbours
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    for (int o = -3; o <= 3; o++) {
        const int t = sc + o;
        if (o == 0 || t < 0 || t >= P) continue;
        insert3(b0, b1, b2, dist2(px, py, pz, sp[3 * (size_t)t], sp[3 * (size_t)t + 1], sp[3 * (size_t)t + 2]));
    }
    const float reject = b2;
    b0 = b1 = b2 = FLT_MAX;
    const int lane = gsr_lane();
    for (int b = 0; b < nbox; b++) {
        // conservative lower bound with the same fmaf chain as dist2 (each |component| <= the true one)
        const float dbox = box_dist2(px, py, pz, boxes + 6 * (size_t)b);
        const bool want = valid && !(dbox > reject || dbox > b2);
        if (__ballot(want) == 0ull) continue;  // wave-uniform: nobody needs this box
        const int start = b * kBox;
        const int end = min(P, start + kBox);
        for (int base = start; base < end; base += 64) {
            const int t = base + lane;
            const bool tv = t < end;
            const int tc = tv ? t : end - 1;
            const float qx = sp[3 * (size_t)tc], qy = sp[3 * (size_t)tc + 1], qz = sp[3 * (size_t)tc + 2];
            const int cnt = min(64, end - base);
            for (int j = 0; j < cnt; j++) {
                const float d = dist2(px, py, pz, bcast(qx, j), bcast(qy, j), bcast(qz, j));
                if (base + j != s) insert3(b0, b1, b2, d);
            }
        }
    }
    if (valid) out[order[s]] = (b0 + b1 + b2) / 3.0f;
}

}  // namespace

extern "C" size_t gsr_knn_workspace_bytes(int32_t P) {
    size_t bytes = 0;
    KnnState::carve(nullptr, P, &bytes);
    return bytes;
}

extern "C" int gsr_knn_dist2(int32_t P, const float *points, float *mean_dist2, void *workspace,
                             size_t workspace_bytes, void *stream_) {
    if (P < 0 || (P > 0 && (!points || !mean_dist2 || !workspace))) {
        gsr_set_error("gsr_knn_dist2: null pointer or negative P");
        return GSR_E_INVALID;
    }
    if (P == 0) return GSR_OK;
    if (workspace_bytes < gsr_knn_workspace_bytes(P)) {
        gsr_set_error("gsr_knn_dist2: workspace too small");
        return GSR_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const KnnState s = KnnState::carve((char *)workspace, P);
    const int nred = min(256, gsr_div_up(P, GSR_BLOCK));
    hipLaunchKernelGGL(knn_minmax_partial_kernel, dim3(nred), dim3(GSR_BLOCK), 0, stream, P, points, s.minmax_partial);
    hipLaunchKernelGGL(knn_minmax_final_kernel, dim3(1), dim3(64), 0, stream, nred, s.minmax_partial, s.minmax, s.n_dev,
                       (uint32_t)P);
    // 30-bit codes, 11 bits per pass = 3 passes: start in side 1 so that the sorted order ends in idx[0]
    const int start = gsr_radix_passes(30, GSR_DEPTH_RADIX_BITS) & 1;
    hipLaunchKernelGGL(knn_morton_kernel, dim3(gsr_div_up(P, GSR_BLOCK)), dim3(GSR_BLOCK), 0, stream, P, points,
                       s.minmax, s.key[start], s.idx[start]);
    if (int e = gsr_check_launch("knn_morton", false, stream)) return e;
    uint32_t *key[2] = {s.key[0], s.key[1]};
    uint32_t *val[2] = {s.idx[0], s.idx[1]};
    if (int e = gsr_radix_sort_u32(key, val, s.n_dev, P, 30, GSR_DEPTH_RADIX_BITS, start, s.sort_table, s.sort_totals,
                                   false, stream))
        return e;
    const int nbox = gsr_div_up(P, kBox);
    hipLaunchKernelGGL(knn_gather_box_kernel, dim3(nbox), dim3(GSR_BLOCK), 0, stream, P, points, s.idx[0],
                       s.sorted_pts, s.boxes);
    hipLaunchKernelGGL(knn_search_kernel, dim3(gsr_div_up(P, GSR_BLOCK)), dim3(GSR_BLOCK), 0, stream, P, s.sorted_pts,
                       s.idx[0], s.boxes, nbox, mean_dist2);
    return gsr_check_launch("knn_search", false, stream);
}
