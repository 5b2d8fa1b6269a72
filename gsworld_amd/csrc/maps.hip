// maps.hip -- per-pixel segmentation and depth maps of a rendered frame (gsr_render_maps, include/gsr.h).
//
// Definition (the contract of every layer above and of tests/test_maps_*.py): a pixel walks the depth-ordered list of its
// 16 x 16 tile exactly as the colour compositor does -- alpha = min(0.99, opacity exp(power)), skipped when power > 0 or
// alpha < 1/255, T <- T (1 - alpha) -- and its MEDIAN CONTRIBUTOR is the first composited Gaussian after which
// T (1 - alpha) < 0.5.  label = (int16)(int)labels[g] and depth = depth_scale / rec[0].w (= depth_scale * view depth) of
// that Gaussian; a pixel whose transmittance never drops below 0.5 gets -1 / 0.0.  The compositor's own stop rule
// (T (1 - alpha) < 1e-4) cannot fire first: alpha <= 0.99 takes T >= 0.5 no lower than 0.005.
//
// The pass runs behind a frame, on the frame's own state, and never touches the colour compositor (render.hip): it reads
//   * the frame header's overflow flag -- a frame whose instances overflowed the binning capacity shows the background, and
//     so do its maps (no host read: the flag is read here, on the device);
//   * the lists: per tile (exact / training-layout frames, every A/B path), or per super-tile (forward_only frames on the
//     default path) with the per-tile membership test the compositor applies there (the tile rect in rec[2].w);
//   * the splat records.  Inference frames keep tau in rec[0].z instead of the view depth; rec[0].w = 1 / depth is written
//     by every preprocess path (preprocess.hip), so the same expression gives the depth in every frame mode.
// Frames that kept blocks of the previous frame (GSR_MODEL_VERSION: preprocess.hip prep_block_cached) leave valid records of
// every listed Gaussian in the state, and frames that reuse tiles (GSR_FRAME_KEPT) still place complete lists for every tile
// -- only the compositor skips the kept ones.  Neither needs a case of its own here.
//
// Shape: a wave per 8 x 8 quadrant (a workgroup per tile), like the compositor's unit.  Per round the wave gathers 64
// candidates, culls them with quadrant_may_hit and compacts the survivors into its private LDS list (ballot + mbcnt rank);
// every lane then replays the survivors in list order for its pixel.  A lane is finished at its median contributor, and
// the wave leaves once a ballot says all 64 pixels are decided -- in most pixels after a few contributors, where the
// compositor goes on to T < 1e-4.  Power and alpha are the compositor's operations: the pre-scaled -A/2, -C/2, -B form of
// render.hip stream_list_put / stream_eval and gsr_exp_power (libgsr_hip_expacc.so links maps_expacc.o, built with
// -DGSR_EXP_ACCURATE=1 as render_expacc.o is), so the 0.5 decision agrees with the colour compositor of the same library.
#include "gsr_internal.h"

namespace {

__global__ __launch_bounds__(GSR_BLOCK) void render_maps_kernel(const GsrBatch<GsrMapsArgs> bt) {
    // per wave, one survivor = 2 x 16 B: (x, y, -A/2, -C/2) | (-B, opacity, 1 / depth, Gaussian index bits)
    __shared__ float4 s_list[GSR_BLOCK / GSR_WAVE][GSR_WAVE][2];
    const GsrMapsArgs &a = bt.f[blockIdx.y];
    const int tiles = a.gx * a.gy;
    if ((int)blockIdx.x >= tiles) return;  // (frames of a launch may differ in size: the grid spans the largest)
    const int lane = gsr_lane(), wave = gsr_wave();
    const int tile = (int)blockIdx.x, quad = wave;
    const uint32_t tx = (uint32_t)(tile % a.gx), ty = (uint32_t)(tile / a.gx);
    const int qx0 = (int)tx * GSR_TILE + ((quad & 1) << 3), qy0 = (int)ty * GSR_TILE + ((quad >> 1) << 3);
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px, pfy = (float)py, qxf = (float)qx0, qyf = (float)qy0;
    float4(*list)[2] = s_list[wave];

    int n_inst = 0;
    const uint32_t *src = a.point_list;
    if (a.hdr->overflow == 0u) {  // (an overflowed frame: background maps, as its RGB shows the background)
        constexpr int kSX = GSR_SUPER_SX, kSY = GSR_SUPER_SY;
        const uint2 range = a.ranges[a.super ? (int)((ty >> kSY) * (uint32_t)((a.gx + (1 << kSX) - 1) >> kSX) + (tx >> kSX))
                                             : tile];
        n_inst = (int)(range.y - range.x);
        src += range.x;
    }
    // the median contributor of this lane's pixel: found = false -> background (-1, 0.0)
    bool done = !inside, found = false;
    float T = 1.0f, inv_depth = 0.0f;
    uint32_t gsel = 0u;

    // global -> register pipeline as in the compositor: records of round rd in (f0, f1, rb), indices of round rd + 1 in g_next
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 f0 = zero4, f1 = zero4;
    uint32_t g_cur = 0u, rb = 0u, g_next = 0u;
    if (lane < n_inst) {
        g_cur = src[lane];
        const float4 *rec = a.splat + 3 * (size_t)g_cur;
        f0 = rec[0];
        f1 = rec[1];
        if (a.super) rb = __float_as_uint(rec[2].w);
    }
    if (GSR_WAVE + lane < n_inst) g_next = src[GSR_WAVE + lane];
    const int rounds = (n_inst + GSR_WAVE - 1) / GSR_WAVE;
    for (int rd = 0; rd < rounds; rd++) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        // ---- cull + compact this round's candidates into the wave's list
        const int p = rd * GSR_WAVE + lane;
        bool keep = p < n_inst;
        if (a.super) {
            // getRect of upstream: rect_min <= tile < rect_max on both axes; tau comes with the record (preprocess.hip)
            keep = keep && tx - (rb & 255u) < ((rb >> 16) & 255u) - (rb & 255u) &&
                   ty - ((rb >> 8) & 255u) < (rb >> 24) - ((rb >> 8) & 255u);
            keep = keep && quadrant_may_hit<true>(f0.x, f0.y, f1, qxf, qyf, 7.0f, f0.z);
        } else {
            keep = keep && quadrant_may_hit(f0.x, f0.y, f1, qxf, qyf);
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        const int n_surv = (int)__builtin_popcountll(mask);
        if (keep) {
            // (the pre-scaled quadratic form of stream_list_put: power = fma((-B) dx, dy, fma((-C/2) dy, dy, ((-A/2) dx) dx)))
            list[rank][0] = make_float4(f0.x, f0.y, -0.5f * f1.x, -0.5f * f1.z);
            list[rank][1] = make_float4(-f1.y, f1.w, f0.w, __uint_as_float(g_cur));
        }
        // ---- next round's gathers go out before the replay so that they fly under it
        {
            const int pn = (rd + 1) * GSR_WAVE + lane;
            f0 = zero4;
            f1 = zero4;
            rb = 0u;
            g_cur = g_next;
            if (pn < n_inst) {
                const float4 *rec = a.splat + 3 * (size_t)g_cur;
                f0 = rec[0];
                f1 = rec[1];
                if (a.super) rb = __float_as_uint(rec[2].w);
            }
            if (pn + GSR_WAVE < n_inst) g_next = src[pn + GSR_WAVE];
        }
        __builtin_amdgcn_wave_barrier();  // (list writes above, list reads below; same wave)
        // ---- replay the survivors in list order
        for (int i = 0; i < n_surv; i++) {
            const float4 e0 = list[i][0], e1 = list[i][1];
            const float dx = e0.x - pfx, dy = e0.y - pfy;
            const float q = __builtin_fmaf(e0.w * dy, dy, (e0.z * dx) * dx);
            const float power = __builtin_fmaf(e1.x * dx, dy, q);
            const float alpha = fminf(0.99f, e1.y * gsr_exp_power(power));
            const bool hit = !done && power <= 0.0f && alpha >= 1.0f / 255.0f;
            const float test_T = T * (1.0f - alpha);
            if (hit) {
                T = test_T;
                if (test_T < 0.5f) {
                    done = true;
                    found = true;
                    inv_depth = e1.z;
                    gsel = __float_as_uint(e1.w);
                }
            }
            if ((i & 7) == 7 && __builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        }
        __builtin_amdgcn_wave_barrier();  // the next round overwrites the list
    }
    if (inside) {
        const size_t pid = (size_t)py * a.W + px;
        if (a.out_label != nullptr) a.out_label[pid] = found ? (int16_t)(int)a.labels[gsel] : (int16_t)-1;
        if (a.out_depth != nullptr) a.out_depth[pid] = found ? a.depth_scale / inv_depth : 0.0f;
    }
}

}  // namespace

// Up to GSR_MAX_FRAMES_PER_LAUNCH frames per launch; grid = (tiles of the largest frame, frames): workgroup t of frame k
// takes tile t's four quadrants.
int gsr_launch_maps(int B, const GsrMapsArgs *frames, bool debug, hipStream_t stream) {
    for (int k0 = 0; k0 < B; k0 += GSR_MAX_BATCH) {
        const int n = B - k0 < GSR_MAX_BATCH ? B - k0 : GSR_MAX_BATCH;
        GsrBatch<GsrMapsArgs> bt{};  // (entries beyond n stay zero: nothing uninitialised travels in the kernarg)
        int tiles = 0;
        for (int k = 0; k < n; k++) {
            bt.f[k] = frames[k0 + k];
            tiles = tiles > bt.f[k].gx * bt.f[k].gy ? tiles : bt.f[k].gx * bt.f[k].gy;
        }
        hipLaunchKernelGGL(render_maps_kernel, dim3(tiles, n), dim3(GSR_BLOCK), 0, stream, bt);
        if (int e = gsr_check_launch("render_maps", debug, stream)) return e;
    }
    return GSR_OK;
}
