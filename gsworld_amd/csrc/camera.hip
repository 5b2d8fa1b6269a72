// camera.hip -- camera records from simulator sensor poses (gsr_cameras_from_extrinsics, include/gsr.h).
//
// Definition (the contract of every layer above and of tests/test_per_env_cameras_*.py).  Per view k the inputs are the
// simulator's OpenCV world->camera extrinsic E = [A | t] (float32, row-major 3 x 4), the caller's rigid_sim2real G (4 x 4)
// and scale s (binary64), and the float32 projection matrix Q = getProjectionMatrix(0.01, 100, FoVx, FoVy)^T (row-major).
// All arithmetic is binary64 in the order written, no contraction (the library builds with -ffp-contract=off); every sum of
// three products is ((x0 y0 + x1 y1) + x2 y2):
//   1. A, t = E[:, :3], E[:, 3];
//   2. Ai = inverse of A by adjugate / det, the cofactor formula of gsr_internal.h gsr_inverse3_f64 (the one the point
//      cloud's C2W uses);
//   3. p_sim_i = -(Ai t)_i * s                                  (the simulator camera's position, scaled);
//   4. Rr = G[:3, :3] Ai,  pr_i = ((G_i0 p0 + G_i1 p1) + G_i2 p2) + G_i3   (the camera-to-world of the scene camera);
//   5. Rw = inverse of Rr (the same adjugate),  tw_i = -(Rw pr)_i        (its world-to-camera W2C = [Rw | tw]);
//   6. world_view = (float)W2C^T: world_view[4 r + c] = W2C[c][r] (W2C's last row 0 0 0 1);
//   7. full_proj[4 r + c] = (float)(((v_r0 Q_0c + v_r1 Q_1c) + v_r2 Q_2c) + v_r3 Q_3c) with v the float32 world_view;
//   8. centre = (float)pr; the record's pad float is written 0.
// The record is world_view (16) | full_proj (16) | centre (3) | pad (1), as gsworld_amd/closed_loop.py's staging vector
// holds a camera and GsrInputs.viewmatrix / projmatrix / campos read it.  This is cam_maniskill2gs + view_params
// (gsworld_amd/camera.py) with the float32 torch steps taken in binary64: the records agree with the reference's own
// cameras to a few float32 ulps (tests/test_per_env_cameras_cpu.py).
//
// Launch: one thread per view, 64 per workgroup; no allocation, no synchronisation (capturable).
#include "gsr_internal.h"

#include <string.h>

namespace {

constexpr int kCamBlock = 64;

struct CamArgs {
    const float *ext;
    const float *proj;
    float *out;
    const int32_t *off;
    double G[16];
    double s;
    int n;
};

__global__ __launch_bounds__(kCamBlock) void cameras_kernel(const CamArgs a) {
    const int k = (int)(blockIdx.x * kCamBlock + threadIdx.x);
    if (k >= a.n) return;
    const float *E = a.ext + (a.off ? a.off[3 * k] : 12 * k);
    const float *Q = a.proj + (a.off ? a.off[3 * k + 1] : 16 * k);
    float *o = a.out + (a.off ? a.off[3 * k + 2] : 36 * k);
    const double A[3][3] = {{E[0], E[1], E[2]}, {E[4], E[5], E[6]}, {E[8], E[9], E[10]}};
    const double t[3] = {E[3], E[7], E[11]};
    double Ai[3][3];
    gsr_inverse3_f64(A, Ai);
    double p[3];
    for (int i = 0; i < 3; i++) p[i] = -((Ai[i][0] * t[0] + Ai[i][1] * t[1]) + Ai[i][2] * t[2]) * a.s;
    double Rr[3][3], pr[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
            Rr[i][j] = (a.G[4 * i + 0] * Ai[0][j] + a.G[4 * i + 1] * Ai[1][j]) + a.G[4 * i + 2] * Ai[2][j];
        pr[i] = ((a.G[4 * i + 0] * p[0] + a.G[4 * i + 1] * p[1]) + a.G[4 * i + 2] * p[2]) + a.G[4 * i + 3];
    }
    double Rw[3][3];
    gsr_inverse3_f64(Rr, Rw);
    float v[16];
    for (int c = 0; c < 3; c++) {
        for (int r = 0; r < 3; r++) v[4 * r + c] = (float)Rw[c][r];
        v[4 * 3 + c] = (float)(-((Rw[c][0] * pr[0] + Rw[c][1] * pr[1]) + Rw[c][2] * pr[2]));
        v[4 * c + 3] = 0.0f;
    }
    v[15] = 1.0f;
    float q[16];
    for (int i = 0; i < 16; i++) q[i] = Q[i];
    for (int i = 0; i < 16; i++) o[i] = v[i];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++)
            o[16 + 4 * r + c] = (float)((((double)v[4 * r + 0] * (double)q[c] + (double)v[4 * r + 1] * (double)q[4 + c]) +
                                         (double)v[4 * r + 2] * (double)q[8 + c]) +
                                        (double)v[4 * r + 3] * (double)q[12 + c]);
    for (int i = 0; i < 3; i++) o[32 + i] = (float)pr[i];
    o[35] = 0.0f;
}

}  // namespace

extern "C" int gsr_cameras_from_extrinsics(const GsrSensorCameras *s, void *stream) {
    if (!s) {
        gsr_set_error("gsr_cameras_from_extrinsics: null spec");
        return GSR_E_INVALID;
    }
    if (s->struct_size != (int32_t)sizeof(GsrSensorCameras)) {
        gsr_set_error("gsr_cameras_from_extrinsics: struct_size %d, this library's GsrSensorCameras has %d bytes",
                      (int)s->struct_size, (int)sizeof(GsrSensorCameras));
        return GSR_E_INVALID;
    }
    if (s->n < 1 || s->n > GSR_CAM_MAX_VIEWS) {
        gsr_set_error("gsr_cameras_from_extrinsics: need 1 <= n <= %d views, got %d", GSR_CAM_MAX_VIEWS, (int)s->n);
        return GSR_E_INVALID;
    }
    if (!s->extrinsic || !s->projection || !s->out) {
        gsr_set_error("gsr_cameras_from_extrinsics: null extrinsic, projection or out");
        return GSR_E_INVALID;
    }
    const double sc = s->scale_sim2real;
    if (!(sc == sc) || sc == 0.0 || sc - sc != 0.0) {
        gsr_set_error("gsr_cameras_from_extrinsics: scale_sim2real must be finite and non-zero");
        return GSR_E_INVALID;
    }
    CamArgs a;
    memset(&a, 0, sizeof(a));
    a.ext = s->extrinsic;
    a.proj = s->projection;
    a.out = s->out;
    a.off = s->offsets;
    for (int i = 0; i < 16; i++) a.G[i] = s->rigid_sim2real[i];
    a.s = sc;
    a.n = s->n;
    hipLaunchKernelGGL(cameras_kernel, dim3(gsr_div_up(s->n, kCamBlock)), dim3(kCamBlock), 0, (hipStream_t)stream, a);
    return gsr_check_launch("cameras_from_extrinsics", false, (hipStream_t)stream);
}
