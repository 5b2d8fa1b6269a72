// train_loss.hip -- gsr_train_loss / gsr_train_loss_backward (include/gsr.h holds the definition): the loss of a 3DGS
// training iteration with upstream's exposure affine, alpha mask, clamp and inverse-depth term, and all of its gradients.
//
// Forward:  prologue (x = clamp(color E) alpha -> scratch; per-workgroup sums of the depth term)  ->  the ssim pass of
// gsr_photometric_loss on x (ssim.hip)  ->  one workgroup adds every partial sum in binary64.
// Backward: the ssim backward pass on x (dL/dx into dL_dcolor)  ->  epilogue, one pixel per thread: recomputes y, applies
// the clamp's gate and alpha, turns dL/dx into dL/dcolor in place, writes dL_dinvdepth and leaves per-workgroup sums of the
// twelve exposure gradients  ->  one workgroup adds those in binary64.
// Without exposure and alpha mask there is no x: the ssim passes read `color` through their own clamp, exactly as
// gsr_photometric_loss(clamp01 = 1) does.  Every kernel streams plane-major rows, one pixel per thread (coalesced dwords).
#include "gsr_internal.h"

namespace {

struct Exposure {
    float e[12];
};

__device__ __forceinline__ Exposure load_exposure(const float *__restrict__ exposure) {
    Exposure E = {};
#pragma unroll
    for (int k = 0; k < 12; k++) E.e[k] = exposure[k];  // (uniform address: scalar loads)
    return E;
}

// y_c = ((c0 E[0][c] + c1 E[1][c]) + c2 E[2][c]) + E[c][3]
__device__ __forceinline__ float expose(const Exposure &E, float c0, float c1, float c2, int c) {
    return ((c0 * E.e[c] + c1 * E.e[4 + c]) + c2 * E.e[8 + c]) + E.e[4 * c + 3];
}

// sum over the 256 threads of a workgroup in a fixed order; the result is valid in thread 0.  s_red: 4 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float *s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (gsr_lane() == 0) s_red[gsr_wave()] = v;
    __syncthreads();
    const float r = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(GSR_BLOCK) void train_loss_prologue_kernel(int HW, const float *__restrict__ color,
                                                                        const float *__restrict__ exposure,
                                                                        const float *__restrict__ alpha,
                                                                        const float *__restrict__ invdepth,
                                                                        const float *__restrict__ mono,
                                                                        const float *__restrict__ depth_mask,
                                                                        float *__restrict__ x,
                                                                        float *__restrict__ depth_partials) {
    __shared__ float s_red[4];
    const int p = (int)blockIdx.x * GSR_BLOCK + (int)threadIdx.x;
    const bool in = p < HW;
    if (x != nullptr && in) {
        const float c0 = color[p], c1 = color[(size_t)HW + p], c2 = color[2 * (size_t)HW + p];
        float y[3] = {c0, c1, c2};
        if (exposure != nullptr) {
            const Exposure E = load_exposure(exposure);
#pragma unroll
            for (int c = 0; c < 3; c++) y[c] = expose(E, c0, c1, c2, c);
        }
        const float a = alpha != nullptr ? alpha[p] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v = y[c] != y[c] ? y[c] : fminf(fmaxf(y[c], 0.f), 1.f);  // (torch.clamp keeps a NaN)
            if (alpha != nullptr) v = v * a;
            x[(size_t)c * HW + p] = v;
        }
    }
    if (depth_partials != nullptr) {
        const float d = in ? fabsf((invdepth[p] - mono[p]) * depth_mask[p]) : 0.f;
        const float s = block_sum(d, s_red);
        if (threadIdx.x == 0) depth_partials[blockIdx.x] = s;
    }
}

// one workgroup: the ssim and |.| partial sums in the order of gsr_photometric_loss's own sum (ssim.hip loss_finish_kernel:
// thread t takes entries t, t + 1024, ... in ascending order, then a halving tree), the depth partials likewise
constexpr int kFinT = 1024;
__global__ __launch_bounds__(kFinT) void train_loss_finish_kernel(const float *__restrict__ partials, int nb, double n,
                                                                  const float *__restrict__ depth_partials, int nbd,
                                                                  double hw, float lambda, float depth_weight,
                                                                  float *__restrict__ loss, float *__restrict__ terms) {
    __shared__ double s_a[kFinT], s_b[kFinT], s_d[kFinT];
    double a = 0.0, b = 0.0, d = 0.0;
    const float2 *pp = reinterpret_cast<const float2 *>(partials);
    for (int i = (int)threadIdx.x; i < nb; i += kFinT) {
        const float2 v = pp[i];
        a += (double)v.x;
        b += (double)v.y;
    }
    if (depth_partials != nullptr)
        for (int i = (int)threadIdx.x; i < nbd; i += kFinT) d += (double)depth_partials[i];
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    s_d[threadIdx.x] = d;
    __syncthreads();
    for (int o = kFinT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_a[threadIdx.x] += s_a[threadIdx.x + o];
            s_b[threadIdx.x] += s_b[threadIdx.x + o];
            s_d[threadIdx.x] += s_d[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double l1 = s_b[0] / n, ssim = s_a[0] / n;
        double total = (1.0 - (double)lambda) * l1 + (double)lambda * (1.0 - ssim);
        double depth = 0.0;
        if (depth_partials != nullptr) {
            depth = s_d[0] / hw;
            total += (double)depth_weight * depth;
        }
        loss[0] = (float)total;
        if (terms != nullptr) {
            terms[0] = (float)total;
            terms[1] = (float)l1;
            terms[2] = (float)ssim;
            terms[3] = (float)depth;
        }
    }
}

// dL_dcolor holds dL/dx (the ssim backward pass, grad_loss folded in) when `do_color`: rewritten in place as dL/dcolor.
// exp_partials: [12][gridDim.x] sums of this workgroup's pixels, entry k as dL_dexposure[k].
__global__ __launch_bounds__(GSR_BLOCK) void train_loss_epilogue_kernel(int HW, const float *__restrict__ color,
                                                                        const float *__restrict__ exposure,
                                                                        const float *__restrict__ alpha,
                                                                        const float *__restrict__ invdepth,
                                                                        const float *__restrict__ mono,
                                                                        const float *__restrict__ depth_mask,
                                                                        const float *__restrict__ grad_loss, float w_depth,
                                                                        int do_color, float *__restrict__ dL_dcolor,
                                                                        float *__restrict__ dL_dinvdepth,
                                                                        float *__restrict__ exp_partials) {
    __shared__ float s_exp[4][12];
    const int p = (int)blockIdx.x * GSR_BLOCK + (int)threadIdx.x;
    const bool in = p < HW;
    if (dL_dinvdepth != nullptr && in) {
        const float gl = grad_loss != nullptr ? grad_loss[0] : 1.0f;
        const float m = depth_mask[p], v = (invdepth[p] - mono[p]) * m;
        const float s = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
        dL_dinvdepth[p] = (w_depth * gl) * s * m;
    }
    if (!do_color) return;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, g[3] = {0.f, 0.f, 0.f};
    Exposure E = {};
    if (exposure != nullptr) E = load_exposure(exposure);
    if (in) {
        c0 = color[p];
        c1 = color[(size_t)HW + p];
        c2 = color[2 * (size_t)HW + p];
        const float a = alpha != nullptr ? alpha[p] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float y = exposure != nullptr ? expose(E, c0, c1, c2, c) : (c == 0 ? c0 : (c == 1 ? c1 : c2));
            float gx = dL_dcolor[(size_t)c * HW + p];
            if (alpha != nullptr) gx = gx * a;
            g[c] = (y >= 0.f && y <= 1.f) ? gx : 0.f;  // (a NaN y stops the gradient, as gsr_photometric_loss)
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float v = exposure != nullptr ? (g[0] * E.e[4 * i] + g[1] * E.e[4 * i + 1]) + g[2] * E.e[4 * i + 2] : g[i];
            dL_dcolor[(size_t)i * HW + p] = v;
        }
    }
    if (exp_partials != nullptr) {
        // the twelve sums of the workgroup: each wave reduces its twelve values by shuffles, one LDS stage, one barrier;
        // thread k adds the four waves' entry k in a fixed order
        const float ci[3] = {c0, c1, c2};
        float v[12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int r = k >> 2, c = k & 3;
            // E[r][c], c < 3: input channel r into output channel c; E[r][3]: the offset of output channel r
            v[k] = c < 3 ? ci[r] * g[c] : g[r];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        }
        if (gsr_lane() == 0) {
#pragma unroll
            for (int k = 0; k < 12; k++) s_exp[gsr_wave()][k] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 12) {
            const int k = (int)threadIdx.x;
            exp_partials[(size_t)k * gridDim.x + blockIdx.x] = (s_exp[0][k] + s_exp[1][k]) + (s_exp[2][k] + s_exp[3][k]);
        }
    }
}

// one workgroup: the twelve exposure sums over the epilogue's workgroups, binary64, fixed order
__global__ __launch_bounds__(GSR_BLOCK) void train_loss_exposure_finish_kernel(const float *__restrict__ exp_partials, int nbp,
                                                                               float *__restrict__ dL_dexposure) {
    __shared__ double s[GSR_BLOCK];
    for (int k = 0; k < 12; k++) {
        double a = 0.0;
        for (int i = (int)threadIdx.x; i < nbp; i += GSR_BLOCK) a += (double)exp_partials[(size_t)k * nbp + i];
        s[threadIdx.x] = a;
        __syncthreads();
        for (int o = GSR_BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) dL_dexposure[k] = (float)s[0];
        __syncthreads();
    }
}

struct Layout {
    size_t nb, nbp, n;
    float *partials, *maps, *x, *depth_partials, *exp_partials;
    size_t floats;
};

// x only with an exposure or an alpha mask, the exposure partials only with an exposure: a plain call needs neither
Layout carve(float *scratch, int H, int W, bool want_x, bool want_exp) {
    Layout l;
    l.n = 3 * (size_t)H * W;
    l.nb = gsr_ssim_loss_blocks(3, H, W);
    l.nbp = (size_t)gsr_div_up((int64_t)H * W, GSR_BLOCK);
    float *p = scratch;
    l.partials = p; p += 2 * l.nb;  // (pairs first: read as float2 -- scratch is 8-byte aligned)
    l.maps = p; p += 3 * l.n;
    l.depth_partials = p; p += l.nbp;
    l.x = p; p += want_x ? l.n : 0;
    l.exp_partials = p; p += want_exp ? 12 * l.nbp : 0;
    l.floats = (size_t)(p - scratch);
    return l;
}
Layout carve(const GsrTrainLoss *a) {
    return carve(a->scratch, a->H, a->W, a->exposure || a->alpha_mask, a->exposure != nullptr);
}

bool size_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 28); }

bool is_finite_f(float v) { return v == v && v - v == 0.f; }

int check_args(const GsrTrainLoss *a, const char *who, bool backward) {
    if (!a || a->struct_size != (int32_t)sizeof(GsrTrainLoss)) {
        gsr_set_error("%s: null argument or struct_size mismatch", who);
        return GSR_E_INVALID;
    }
    if (!size_ok(a->H, a->W)) {
        gsr_set_error("%s: H and W must be positive with H W <= 2^28", who);
        return GSR_E_INVALID;
    }
    if (!a->color || !a->target || !a->scratch || (!backward && !a->loss)) {
        gsr_set_error("%s: null pointer", who);
        return GSR_E_INVALID;
    }
    const int depth_parts = (a->invdepth != nullptr) + (a->mono_invdepth != nullptr) + (a->depth_mask != nullptr);
    if (depth_parts != 0 && depth_parts != 3) {
        gsr_set_error("%s: invdepth, mono_invdepth and depth_mask come together or not at all", who);
        return GSR_E_INVALID;
    }
    if (!is_finite_f(a->lambda_dssim) || !is_finite_f(a->depth_weight)) {
        gsr_set_error("%s: lambda_dssim and depth_weight must be finite", who);
        return GSR_E_INVALID;
    }
    if (a->scratch_floats < 0 || (size_t)a->scratch_floats < carve(a).floats) {
        gsr_set_error("%s: scratch is smaller than gsr_train_loss_scratch_needed says for this call", who);
        return GSR_E_INVALID;
    }
    if ((uintptr_t)a->scratch % 8 != 0) {
        gsr_set_error("%s: scratch must be 8-byte aligned", who);
        return GSR_E_INVALID;
    }
    if (backward && (!a->dL_dcolor || (depth_parts == 3 && !a->dL_dinvdepth) || (a->exposure && !a->dL_dexposure))) {
        gsr_set_error("%s: null gradient pointer", who);
        return GSR_E_INVALID;
    }
    return GSR_OK;
}

}  // namespace

extern "C" size_t gsr_train_loss_scratch_floats(int32_t H, int32_t W) {
    if (!size_ok(H, W)) return 0;
    return carve(nullptr, H, W, true, true).floats;
}

extern "C" size_t gsr_train_loss_scratch_needed(const GsrTrainLoss *a) {
    if (!a || a->struct_size != (int32_t)sizeof(GsrTrainLoss) || !size_ok(a->H, a->W)) return 0;
    return carve(a).floats;
}

extern "C" int gsr_train_loss(const GsrTrainLoss *a, void *stream_) {
    if (int e = check_args(a, "gsr_train_loss", false)) return e;
    hipStream_t stream = (hipStream_t)stream_;
    const int H = a->H, W = a->W, HW = H * W;
    const Layout l = carve(a);
    const bool plain = !a->exposure && !a->alpha_mask, depth = a->invdepth != nullptr;
    if (!plain || depth) {
        hipLaunchKernelGGL(train_loss_prologue_kernel, dim3((unsigned)l.nbp), dim3(GSR_BLOCK), 0, stream, HW, a->color,
                           a->exposure, a->alpha_mask, a->invdepth, a->mono_invdepth, a->depth_mask,
                           plain ? (float *)nullptr : l.x, depth ? l.depth_partials : (float *)nullptr);
        if (int e = gsr_check_launch("train_loss (prologue)", false, stream)) return e;
    }
    if (int e = gsr_launch_ssim_loss_forward(3, H, W, plain ? a->color : l.x, a->target, a->keep_for_backward, plain ? 1 : 0,
                                             l.maps, l.partials, stream))
        return e;
    hipLaunchKernelGGL(train_loss_finish_kernel, dim3(1), dim3(kFinT), 0, stream, (const float *)l.partials, (int)l.nb,
                       (double)l.n, depth ? (const float *)l.depth_partials : (const float *)nullptr, (int)l.nbp, (double)HW,
                       a->lambda_dssim, a->depth_weight, a->loss, a->terms);
    return gsr_check_launch("train_loss (sum)", false, stream);
}

extern "C" int gsr_train_loss_backward(const GsrTrainLoss *a, void *stream_) {
    if (int e = check_args(a, "gsr_train_loss_backward", true)) return e;
    hipStream_t stream = (hipStream_t)stream_;
    const int H = a->H, W = a->W, HW = H * W;
    const Layout l = carve(a);
    const bool plain = !a->exposure && !a->alpha_mask, depth = a->invdepth != nullptr;
    const float w_ssim = (float)(-(double)a->lambda_dssim / (double)l.n);
    const float w_l1 = (float)((1.0 - (double)a->lambda_dssim) / (double)l.n);
    if (int e = gsr_launch_ssim_loss_backward(3, H, W, plain ? a->color : l.x, a->target, a->grad_loss, l.maps, w_ssim, w_l1,
                                              plain ? 1 : 0, a->dL_dcolor, stream))
        return e;
    if (!plain || depth) {
        const float w_depth = (float)((double)a->depth_weight / (double)HW);
        hipLaunchKernelGGL(train_loss_epilogue_kernel, dim3((unsigned)l.nbp), dim3(GSR_BLOCK), 0, stream, HW, a->color,
                           a->exposure, a->alpha_mask, a->invdepth, a->mono_invdepth, a->depth_mask, a->grad_loss, w_depth,
                           plain ? 0 : 1, a->dL_dcolor, depth ? a->dL_dinvdepth : (float *)nullptr,
                           a->exposure ? l.exp_partials : (float *)nullptr);
        if (int e = gsr_check_launch("train_loss (epilogue)", false, stream)) return e;
    }
    if (a->exposure) {
        hipLaunchKernelGGL(train_loss_exposure_finish_kernel, dim3(1), dim3(GSR_BLOCK), 0, stream,
                           (const float *)l.exp_partials, (int)l.nbp, a->dL_dexposure);
        return gsr_check_launch("train_loss (exposure sums)", false, stream);
    }
    return GSR_OK;
}
