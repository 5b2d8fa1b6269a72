/*
 * gsr.h -- C ABI of the MI355X-native 3D-Gaussian-Splatting rasterizer (libgsr_hip.so).
 *
 * This is the drop-in boundary under the Python packages GSWorld imports
 * (/root/reference/gsworld/mani_skill/utils/wrappers/gs_world_wrapper.py:11-13,22-26,266-267).  Each entry
 * point names the upstream pybind function of the un-vendored CUDA extension it replaces:
 *
 *   gsr_forward            <->  diff_gaussian_rasterization._C.rasterize_gaussians
 *   gsr_forward_batch      <->  the wrapper's double loop of render() calls per step (gs_world_wrapper.py:238-267)
 *   gsr_backward           <->  diff_gaussian_rasterization._C.rasterize_gaussians_backward
 *   gsr_mark_visible       <->  diff_gaussian_rasterization._C.mark_visible
 *   gsr_knn_dist2          <->  simple_knn._C.distCUDA2
 *   gsr_ssim_forward       <->  fused_ssim_cuda.fusedssim
 *   gsr_ssim_backward      <->  fused_ssim_cuda.fusedssim_backward
 *   gsr_transform_gaussians<->  the per-step rigid transform of GSWorld itself
 *                               (gs_world_wrapper.py:110-162,244-265 + gsworld/utils/gs_utils.py:283-385)
 *   gsr_render_maps        <->  the segmentation / depth observations (obs_mode rgb+segmentation, rgbd) that the wrapper
 *                               leaves to SAPIEN's meshes (gs_world_wrapper.py:184,196,222 overwrite 'rgb' only): here
 *                               from the splatted scene itself, consistent with the frame
 *   gsr_render_pointcloud  <->  the point-cloud observation (obs_mode pointcloud) the wrapper also leaves to SAPIEN's
 *                               meshes, plus the crop / FPS step point-cloud policies run after it: world-frame points
 *                               from the maps, the frame and the camera, sampled to a fixed size on the device
 *   gsr_cameras_from_extrinsics <->  cam_maniskill2gs (gs_world_wrapper.py:277-325), per environment and camera, on the
 *                               device from the simulator's extrinsic_cv
 *
 * Conventions: plain pointers and sizes only (no torch types); every data pointer is DEVICE memory on the
 * current HIP device unless marked [host]; all inputs are borrowed, contiguous, float32; `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Functions return 0 on success or a negative
 * GSR_E_* code; gsr_last_error() returns a human-readable message for the calling thread.
 * Work buffers are caller-owned and grown through a resize callback -- the same contract as upstream's
 * std::function<char*(size_t)> lambdas that resize_ a torch byte tensor and hand back its data_ptr.
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_E_INVALID (-1)   /* bad argument (shape / null / unsupported value) */
#define GSR_E_HIP (-2)       /* a HIP runtime call or kernel failed (debug mode checks every launch) */
#define GSR_E_ALLOC (-3)     /* a resize callback returned NULL */
#define GSR_E_OVERFLOW (-4)  /* num_rendered exceeded the binning capacity in no-sync mode */
#define GSR_E_TRUNCATED (-5) /* a cooperative quadrant of the compositor gave up on a hand-off: pixels of the frame are wrong */

#define GSR_TILE 16          /* BLOCK_X = BLOCK_Y of cuda_rasterizer/config.h */
#define GSR_NEAR_PLANE 0.05f /* /root/reference/README.md:33 (stock upstream 0.2f) */

/* GaussianRasterizationSettings (the 13-field NamedTuple) minus the tensors, plus GSWorld's near plane. */
typedef struct GsrSettings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t sh_degree;    /* active degree D, 0..3 */
    int32_t sh_coeffs;    /* M = coefficients stored per Gaussian (shs is (P, M, 3)) */
    int32_t prefiltered;
    int32_t antialiasing;
    int32_t debug;        /* sync + error check after every kernel */
    float near_plane;     /* cull p_view.z <= near_plane; GSR_NEAR_PLANE for GSWorld */
    /* A/B and test selectors; 0 = the library's default everywhere.  They travel with the call -- the library keeps
     * no mutable process state, so renderers on different threads or devices cannot disturb each other.  Every
     * choice produces the same point list and bit-identical image state.
     * binning_path: 0 = global depth sort + counting placement by tile rows (rows up to 256 tiles; by chunks of depth
     *   ranks beyond), 1 = global depth sort + emit + tile-id radix sort (always used for tile grids above 16384 tiles
     *   or wider than 2048 tiles), 2 = unordered binning + per-tile (depth, index) sort in LDS, 3 = global depth sort +
     *   counting placement by chunks of 256 depth ranks.
     * render_variant: 0 = wave-decoupled culling kernel, 1 = LDS-staged per tile (upstream's structure), 2 = batched
     *   tile kernel, 3 = the same with per-quadrant instance culling.
     * render_blocks_per_cu: 1..8 sizes the persistent grid of the compositing kernel (0 = 6). */
    int32_t binning_path;
    int32_t render_variant;
    int32_t render_blocks_per_cu;
    /* depth_sort: 0 = sample sort (5 launches: per-frame plan, compaction + classification, column sums, stable
     *   partition, per-bucket LDS radix), 1 = 3-pass LSD radix sort over all visible Gaussians (10 launches).  Same depth
     *   order. */
    int32_t depth_sort;
    /* render_split: what the compositor does with the quadrants that were costliest in the previous frame on the same
     *   state (image state bit-identical in every mode).  0 = default: inference frames give each of them a workgroup of
     *   its own -- three waves cull the quadrant's candidates, the fourth composites the survivors; 1 = two 8x4 halves on
     *   two waves (measured slower, kept for A/B); 2 = as 0; 3 = one wave per quadrant, always. */
    int32_t render_split;
    /* forward_only: 1 = inference frame (GSWorld's closed loop never runs a backward: gs_world_wrapper.py:266-270 keeps
     * ["render"] only).  The image is bit-identical to forward_only = 0; what changes is the work behind it:
     *   - preprocess writes nothing a backward would read (cov3D, SH clamp flags, tiles_touched) and GsrOutputs.radii
     *     may be NULL;
     *   - instances are binned per SUPER-TILE of 2 x 1 tiles (32 x 16 px) instead of per tile, and a Gaussian is listed
     *     only where it can colour a pixel: its tile rect is the reference's (getRect) cut down to the bounding box of
     *     the ellipse alpha >= 1/255 (a Gaussian below 1/255 everywhere is listed nowhere) -- 0.47 of the reference's
     *     instances to count, place and fetch at config 2.  The compositor applies that per-tile membership test to
     *     every candidate itself, so every pixel composites the depth-ordered list of ITS 16 x 16 tile minus entries
     *     every one of its pixels would have skipped: the same image bit for bit;
     *   - final_T / n_contrib (read by the backward only) are not written.
     * The state buffers of such a frame are NOT valid inputs of gsr_backward, and gsr_state_view / GsrFrameStats then
     * describe those lists (num_rendered = super-tile instances, num_visible = Gaussians listed somewhere).  Tile grids
     * wider or higher than 255 tiles keep per-tile lists. */
    int32_t forward_only;
} GsrSettings;

typedef struct GsrInputs {
    int32_t P;                   /* number of Gaussians */
    const float *background;     /* (3) */
    const float *means3D;        /* (P,3) */
    const float *shs;            /* (P,M,3) or NULL when colors_precomp is given */
    const float *colors_precomp; /* (P,3) or NULL */
    const float *opacities;      /* (P) */
    const float *scales;         /* (P,3) or NULL when cov3D_precomp is given */
    const float *rotations;      /* (P,4) (r,x,y,z), used un-normalised */
    const float *cov3D_precomp;  /* (P,6) or NULL */
    const float *viewmatrix;     /* (16) world->view, element [r][c] at m[c*4+r] */
    const float *projmatrix;     /* (16) full projection, same layout */
    const float *campos;         /* (3) */
    /* Optional split SH storage (forward only).  3DGS keeps the SH coefficients as two parameters, features_dc
     * (P,1,3) and features_rest (P,M-1,3), and upstream's render() concatenates them for every frame
     * (gaussian_renderer/__init__.py `shs = pc.get_features`: a 2 x 192 B/Gaussian copy, 564 MB of traffic at
     * 1.47 M Gaussians).  When shs_rest is not NULL, `shs` is features_dc and `shs_rest` is features_rest; the
     * colours are bit-identical to the concatenated call.  NULL = upstream layout. */
    const float *shs_rest;       /* (P,M-1,3) or NULL */
    /* Optional raw parameter space (forward only): OR of GSR_RAW_* -- the activations upstream's GaussianModel
     * getters apply per frame (scene/gaussian_model.py: torch.sigmoid / torch.exp / F.normalize, three passes over
     * the model) are then evaluated inside preprocess, in the float32 order fixed by oracle/gs_oracle.c
     * (gso_activate_params; exp = 2^n * Cephes polynomial, ~1 ulp).  0 = upstream contract (activated inputs). */
    int32_t param_space;
    /* Optional rigid transform of labelled Gaussians applied INSIDE preprocess (forward only): what
     * gsr_transform_gaussians computes, without materialising transformed (P,.) buffers -- a frame of environment e from
     * camera c reads the one base model plus environment e's 17-float pose table (see gsr_transform_gaussians below for
     * the table and the arithmetic; the results are bit-identical to transforming first and rendering the outputs).
     * part_labels NULL = off.  part_rescale ((K) bytes or NULL) marks the parts whose log-scales the reference rewrites
     * (needs GSR_RAW_SCALES). */
    const float *part_labels;      /* (P) semantic label per Gaussian, or NULL */
    const int32_t *part_lut;       /* (part_lut_size) label -> part index, -1 = not a moving part */
    int32_t part_lut_size;
    const float *part_transforms;  /* (part_count, 17) */
    int32_t part_count;
    const uint8_t *part_rescale;   /* (part_count) or NULL */
    /* Optional view-frustum culling by blocks of 256 consecutive Gaussians (gsworld_amd/layout.py builds both arrays
     * once per model).  The reference projects every Gaussian in front of the near plane and only then finds that its
     * tile rect is empty (forward.cu preprocessCUDA / getRect): at configs[1] that is 88 % of the model.  cull_blocks
     * holds, per block b of Gaussians [256 b, 256 b + 256), eight floats: the axis-aligned box of their centres
     * (lo.xyz, hi.xyz), rho >= sqrt(largest eigenvalue of every 3D covariance in the block, at scale_modifier 1) and
     * the block's common part label (NaN: labels differ -- such a block is never culled while part_labels is given).
     * A block is skipped only when the box, moved by its part's pose and grown by a rigorous bound of the projected
     * 3-sigma radius, lies wholly behind the near plane or beside the tile grid -- every Gaussian in it then has
     * radii == 0 in the reference as well, so images, radii and lists are bit-identical (preprocess.hip
     * prep_block_culled).  The bounds are the caller's promise: a box that does not contain its Gaussians drops them.
     * Correct for ANY order of the model; tight when neighbours in the model are neighbours in space, hence:
     * orig_index ((P) or NULL): the model arrays are a PERMUTED copy of the caller's model (Morton order per part) and
     * Gaussian i of them is number orig_index[i] of the original.  `radii` is written in ORIGINAL numbering and depth
     * ties resolve by original number, exactly as without the permutation, so the image is the same bit for bit; the
     * opaque state (and the point list in it) stays in the numbering of the permuted arrays.  forward_only frames on the
     * default sort / placement path only. */
    const float *cull_blocks;      /* (ceil(P / 256), 8) or NULL */
    const int32_t *orig_index;     /* (P) or NULL */
    /* Optional appearance transform (forward only: a frame without GsrSettings.forward_only that sets it is refused,
     * GSR_E_INVALID): per-group colour affines applied inside preprocess, for visual domain randomization per environment
     * and episode without a model copy.  Gaussian i belongs to group k = appearance_lut[label] with label =
     * (int)appearance_labels[i] (or (int)part_labels[i] when appearance_labels is NULL); a label outside the LUT, or a LUT
     * entry outside [0, G), is group 0 (the "rest").  Row k of `appearance` is the row-major 3 x 4 affine [M | t], and the
     * colour preprocess computed (max(sh + 0.5, 0), or colors_precomp) becomes, per channel j = r, g, b,
     *     c'_j = max(((M[j][0] r + M[j][1] g) + M[j][2] b) + t[j], 0)
     * in round-to-nearest binary32 multiplies and adds in exactly this order, never contracted to an FMA (no upper clamp:
     * out_rgb8 clamps at 255, out_color keeps the value).  The identity row gives the same colour bit for bit (c >= 0).
     * appearance_versions (G + 1 words, or NULL) drives the block cache of GSR_MODEL_VERSION frames: word k < G describes
     * row k, word G the whole table.  Nonzero G with versions is the caller's promise, in the style of GSR_MODEL_VERSION, that
     * a row whose floats differ from the previous frame's on this state comes with a different word k AND a different word G;
     * a block of one label then keeps its records while its group's word is unchanged, a block of several labels while the
     * table's word is, and the tiles of every recomputed block are composited again (GSR_FRAME_KEPT).  NULL versions: every
     * block is recomputed.  The LUT and the label array are not covered by the words: like part_lut and part_labels they fall
     * under the GSR_MODEL_VERSION promise -- rewriting either in place under an unchanged model version gives stale blocks
     * (pick a new model version, or new arrays, when they change).  The arrays (table, LUT, labels) are read when the frame
     * runs.
     * appearance == NULL and appearance_groups == 0: off (the frame is what it was without these fields).  Otherwise
     * 1 <= appearance_groups <= GSR_APPEARANCE_MAX_GROUPS, a non-NULL LUT with appearance_lut_size >= 1 and a label array are
     * required (else GSR_E_INVALID). */
    const float *appearance;             /* (appearance_groups, 12) or NULL */
    const int32_t *appearance_lut;       /* (appearance_lut_size) label -> group */
    int32_t appearance_lut_size;
    int32_t appearance_groups;           /* G */
    const uint32_t *appearance_versions; /* (G + 1) or NULL */
    const float *appearance_labels;      /* (P) or NULL: part_labels */
} GsrInputs;
#define GSR_APPEARANCE_MAX_GROUPS 64

#define GSR_RAW_OPACITY 1   /* opacities are logits:        opacity  = 1 / (1 + exp(-x)) */
#define GSR_RAW_SCALES 2    /* scales are log-scales:        scale    = exp(x) */
#define GSR_RAW_ROTATIONS 4 /* rotations are un-normalised:  rotation = q / max(|q|, 1e-12) */
/* Bits 8..31 of param_space: a MODEL VERSION, or 0.  Nonzero is the caller's promise that the model arrays (means3D, shs, shs_rest,
 * opacities, scales, rotations), part_labels, part_lut, part_rescale, cull_blocks, orig_index, appearance_lut and appearance_labels
 * hold exactly what they held in the previous frame on this state that carried the same version -- pick a fresh random value whenever
 * any of them is written.
 * Inference frames (GsrSettings.forward_only, default path, radii == NULL) with part_labels and cull_blocks then leave a block of
 * 256 Gaussians as the previous frame on the state computed it when nothing the block's records depend on has changed: settings,
 * camera (view, projection, centre: bit for bit) and the pose row of the block's one part (csrc/preprocess.hip
 * prep_block_cached).  A fixed sensor camera over a scene in which only the robot moves recomputes the robot.  Frames are the same
 * bit for bit; the promise is the caller's: arrays changed under an unchanged version give stale blocks. */
#define GSR_MODEL_VERSION(v) ((int32_t)(((uint32_t)(v) & 0xFFFFFFu) << 8))
/* Bit 3 of param_space, read only beside a model version: the caller's promise that GsrOutputs.out_rgb8 still holds, byte for
 * byte, what the previous frame on this state wrote there (nobody drew into it, nobody else rendered into it).  An inference
 * frame whose ONLY output is out_rgb8 (out_color == out_invdepth == NULL) then leaves a 16 x 16 tile as it stands when camera,
 * background, settings and buffer are the previous frame's and no Gaussian of a recomputed block touches the tile now or touched
 * it then: its list holds the same records in the same order, so the compositor would write the bytes that are there
 * (csrc/render.hip "tile reuse"; preprocess marks the tiles of every recomputed Gaussian).  Frames are the same bit for bit. */
#define GSR_FRAME_KEPT 8

typedef struct GsrOutputs {
    /* The two float images.  Both may be NULL for an inference frame (GsrSettings.forward_only on the default path) that
     * hands over out_rgb8: GSWorld keeps the uint8 frame only (gs_world_wrapper.py:266-270 -- ["render"], x 255, clamp,
     * uint8), and 16 bytes per pixel that nobody reads are then not written (4.9 MB per 640 x 480 frame). */
    float *out_color;    /* (3,H,W) */
    float *out_invdepth; /* (1,H,W) */
    int32_t *radii;      /* (P) */
    /* Optional: the frame as GSWorld consumes it (gs_world_wrapper.py:268-270), (H,W,3) uint8 =
     * (uint8)clamp(255 * out_color, 0, 255), written by the compositor itself instead of a second pass over the
     * image (gsr_pack_rgb8 remains for callers that convert later).  NULL = not wanted. */
    uint8_t *out_rgb8;
    /* Optional: two words the HOST can read and the device can write -- the device-visible address of pinned host memory
     * (gsr_pinned_device_address) or plain device memory.  The frame's capacity check leaves there what GsrFrameStats
     * reports as overflow_frames, as (0x0F10F10F, count) -- (anything else, -) while the state has never overflowed:
     * a caller that runs ahead of the device learns of an overflowed frame without a copy behind every frame (8 bytes,
     * but a copy: ~3 us of the stream per frame) and without a wait.  NULL = not wanted. */
    uint32_t *overflow_mirror;
} GsrOutputs;

/* resize callback: must return a device pointer to at least `bytes` bytes (256-byte aligned), or NULL. */
typedef char *(*gsr_resize_fn)(void *user, size_t bytes);

typedef struct GsrBuffers {
    gsr_resize_fn geom_resize;    void *geom_user;    /* geometry state   (per Gaussian) */
    gsr_resize_fn binning_resize; void *binning_user; /* binning state    (per rendered instance) */
    gsr_resize_fn image_resize;   void *image_user;   /* image state      (per pixel / per tile) */
} GsrBuffers;

/* Frame statistics, all produced by the pipeline itself (N, V, R). */
typedef struct GsrFrameStats {
    int64_t num_visible;  /* V: Gaussians with radii > 0 */
    int64_t num_rendered; /* R: sum of tiles touched */
    int32_t overflow;     /* 1 if R exceeded the binning capacity (no-sync mode only) */
    int32_t overflow_frames; /* how many frames rendered on this geometry state overflowed since the first 256 bytes of
                              * the buffer were last zeroed (this package's resize callbacks zero them on new storage;
                              * a header that never held a count reads as 0) -- a rollout that never synchronises reads
                              * it once at the end to learn whether every frame was valid.  Occupies former padding. */
    int32_t truncated;       /* 1: a cooperative quadrant of THIS frame's compositor timed out waiting for a hand-off between
                              * its waves and was written truncated (cannot happen by the counters' construction; if it ever
                              * does the frame says so instead of showing a wrong quadrant silently: re-render) */
    int32_t coop_timeouts;   /* such quadrants in all frames on this state since the header was last zeroed */
} GsrFrameStats;

const char *gsr_last_error(void);
const char *gsr_version(void);
/* ABI handshake for bindings that mirror the structs above (ctypes, the compiled torch extension): sizes of
 * GsrSettings, GsrInputs, GsrOutputs, GsrBuffers, GsrBackwardInputs, GsrGrads as THIS library was compiled. */
void gsr_abi_sizes(int32_t out[6]);

/* Bytes needed for each state buffer. */
size_t gsr_geom_bytes(int32_t P, int32_t width, int32_t height);
size_t gsr_binning_bytes(int64_t r_capacity);
size_t gsr_image_bytes(int32_t width, int32_t height);

/*
 * Forward rasterization (upstream RasterizeGaussiansCUDA -> CudaRasterizer::Rasterizer::forward).
 *
 * r_capacity <= 0 : exact mode.  One host read-back of num_rendered in the middle of the frame (what
 *                   upstream does), binning state sized exactly; `stats` (may be NULL) is filled.
 * r_capacity  > 0 : no-sync mode.  Binning state sized for r_capacity instances, nothing is read back and the
 *                   call returns as soon as the work is enqueued.  Call gsr_frame_stats() later to learn
 *                   V, R and whether R overflowed the capacity (then the image is invalid: re-run bigger).
 */
int gsr_forward(const GsrSettings *settings, const GsrInputs *in, const GsrOutputs *out,
                const GsrBuffers *buffers, int64_t r_capacity, GsrFrameStats *stats, void *stream);

/*
 * B frames of ONE step in one set of launches: what GSWorld's render loop asks for per simulation step --
 * `for cam_name, cam_param in self.camera_params.items(): for i in range(self.num_envs): render(...)`
 * (gs_world_wrapper.py:238-267; SURVEY.md 8f-4 "render_batch(cameras[B])").  Frame k is described by settings[k], in[k],
 * out[k], buffers[k], r_capacity[k] exactly as gsr_forward takes them: its own camera, pose table, outputs and state
 * buffers; the model arrays are usually shared.  Consecutive frames that (a) take the default path (GsrSettings selectors
 * 0) with a capacity (r_capacity[k] > 0: no mid-frame read-back), (b) have the same P, image size, SH layout and
 * forward_only flag, go through every stage TOGETHER: each of the frame's eleven kernels is launched once with a grid
 * that spans the frames (the per-frame argument blocks travel in the kernarg segment, at most GSR_MAX_FRAMES_PER_LAUNCH
 * frames per set of launches; longer runs are cut into such sets).  The stages of a 640 x 480 frame that are chains of
 * dependent round trips on a few hundred workgroups (compaction, bucket sort, range scans) then fill the chip with
 * B x the workgroups instead of being overlapped by hand on B streams, and the compositor's tail -- its costliest
 * quadrants running alone -- is filled by the next frame's workgroups.  Any other frame (exact mode, A/B selectors,
 * P == 0, another image size) runs by itself as gsr_forward would run it, in the order given; every frame's outputs and
 * state are bit-identical to a gsr_forward call with the same arguments.  Nothing is read back; gsr_frame_stats() on each
 * frame's geometry state tells V, R and overflow afterwards.
 */
#define GSR_MAX_FRAMES_PER_LAUNCH 8
int gsr_forward_batch(int32_t B, const GsrSettings *settings, const GsrInputs *in, const GsrOutputs *out,
                      const GsrBuffers *buffers, const int64_t *r_capacity, void *stream);

/*
 * How gsr_forward would run a frame with these settings on a model of P Gaussians (`permuted`: GsrInputs.orig_index
 * given; r_capacity as for gsr_forward) -- the library's own decision, made on the host without touching a device:
 * out[0] = binning mode (1 = depth sort + counting placement, 2 = bin-then-sort, 0 = depth sort + radix), out[1] = the
 * counting placement (1 by tile rows, 2 by chunks, 0 neither), out[2] = 1: inference frame (forward_only honoured),
 * out[3] = 1: super-tile lists, out[4] = 1: lean state layout, out[5] = 1: LSD radix depth sort (depth_sort = 1, or a
 * model beyond the sample sort's 8 388 608 Gaussians), out[6] = 1: the compositor's order is dealt beside the depth
 * sort, out[7] = 1: exact mode.  Returns GSR_E_INVALID where gsr_forward would (a permuted model on a path that does not
 * take one).
 */
int gsr_plan_query(const GsrSettings *settings, int32_t P, int32_t permuted, int64_t r_capacity, int32_t out[8]);

/* Tuning aid: cycle stamps of the depth-sort kernels (meaningful in builds with -DGSR_SS_TIMING only).  A negative
 * height reads the state of a forward_only frame (the lean layout). */
int gsr_debug_ss_stamps(int32_t P, int32_t width, int32_t height, const void *geom, uint64_t *out64);

/* Tests and tools: what the sample sort of the last frame on `geom` did (synchronises `stream`).  out[0] = 1: it took
 * the kept splitters unchecked (fixed camera, scene standing still); out[1] = 1: it drew new splitters from samples;
 * (both 0: it checked the kept ones against samples and kept them); out[2] = 1: a depth bucket came out above what
 * quantiles of an unchanged scene give; out[3]: consecutive balanced frames on kept splitters before this one; out[4]:
 * depth buckets of the frame; out[5] = 2: it took every second entry of a kept table of twice as many quantiles;
 * out[6]: quadrants the frame's compositor handed to cooperative workgroups; out[7]: reserved (0). */
int gsr_debug_sort_state(const void *geom, int32_t out[8], void *stream);

/* Reads V / R / overflow of the frame whose geometry state is `geom` (synchronises `stream`).  Returns GSR_E_OVERFLOW for a
 * frame that exceeded its capacity, GSR_E_TRUNCATED for one with a timed-out cooperative quadrant (stats filled either way). */
int gsr_frame_stats(const void *geom, GsrFrameStats *stats, void *stream);

/* Views into the opaque state, for tests and tools (device pointers into the caller's buffers). */
typedef struct GsrStateView {
    const float *splat;           /* (P,12): xy, depth, 1/depth | conic xyz, opacity | rgb, radius */
    const float *cov3D;           /* (P,6) */
    const uint8_t *clamped;       /* (P,4) */
    const uint32_t *tiles_touched;/* (P) */
    const uint16_t *rects;        /* (P,4) min.x min.y max.x max.y */
    const uint32_t *depth_order;  /* (V) Gaussian indices, ascending (depth bits, index) */
    const uint32_t *point_list;   /* (R) Gaussian index per instance, tile-major / depth / index order */
    const uint32_t *point_tiles;  /* always NULL: tile ids follow from `ranges` */
    const uint32_t *ranges;       /* (tiles,2) */
    const float *final_T;         /* (H*W) */
    const uint32_t *n_contrib;    /* (H*W) */
} GsrStateView;
int gsr_state_view(int32_t P, int32_t width, int32_t height, int64_t r_capacity_or_R, const void *geom,
                   const void *binning, const void *image, GsrStateView *view);

/*
 * Segmentation and depth maps of rendered frames, from the frames' own state (one pass behind the frames, on `stream`; the
 * colour compositor is not touched).  A pixel walks the depth-ordered list of its 16 x 16 tile as the compositor does --
 * alpha = min(0.99, opacity exp(power)), skipped when power > 0 or alpha < 1/255, T <- T (1 - alpha) -- and its MEDIAN
 * CONTRIBUTOR is the first composited Gaussian after which T (1 - alpha) < 0.5:
 *   out_label[pixel] = (int16)(int)labels[g] of it, or -1 where the transmittance never drops below 0.5;
 *   out_depth[pixel] = depth_scale / (1 / view depth) of it, or 0.0 there (ManiSkill's background depth).
 * Labels are numbered as the arrays the frame was rendered from (a permuted copy when GsrInputs.orig_index was given).  A
 * frame that overflowed its binning capacity gets background maps, as its image shows the background (read on the device:
 * nothing is read back).  No allocation, no synchronisation: the call can be captured into a hipGraph.  Frame k is
 * described by frames[k]; B frames go through launches of up to GSR_MAX_FRAMES_PER_LAUNCH frames.  Every frame the default
 * path of gsr_forward / gsr_forward_batch rendered is accepted (exact or capacity mode, forward_only or not, permuted or
 * not); the state's layout follows from the same plan gsr_forward makes (gsr_plan_query), and a frame gsr_forward would
 * refuse is refused (GSR_E_INVALID).  A frame with P == 0 gets background maps.
 */
typedef struct GsrMapFrame {
    int32_t struct_size;            /* sizeof(GsrMapFrame): the library rejects a mismatch (GSR_E_INVALID) */
    const GsrSettings *settings;    /* [host] as the frame was rendered */
    int32_t P; int32_t permuted;    /* permuted: GsrInputs.orig_index was given */
    int64_t r_capacity;             /* as passed to gsr_forward / gsr_forward_batch (<= 0: exact mode) */
    const void *geom, *binning, *image;  /* the frame's state buffers */
    const float *labels;            /* (P) or NULL (then out_label must be NULL) */
    float depth_scale;
    int16_t *out_label;             /* (H,W) or NULL */
    float *out_depth;               /* (H,W) or NULL */
} GsrMapFrame;
int gsr_render_maps(int32_t B, const GsrMapFrame *frames, void *stream);

/*
 * Optional stage timing with HIP events recorded on the caller's stream (what bench.py's roofline uses).
 * mode 0 = off, 1 = the compositing kernel only (2 events / frame), 2 = every stage (6 events / frame).
 * Stages: 0 preprocess, 1 depth sort (compaction, partition, buckets), 2 tile counts -> ranges (band ranges, count,
 * scan, tile starts; the fallback paths: tile offsets), 3 placement of the instances (fallback: emit + tile sort +
 * ranges), 4 render.
 * The recorder is per calling thread (enable, render and collect from the same thread); at most 4096 frames
 * are recorded between two collects.
 */
#define GSR_PROFILE_STAGES 5
typedef struct GsrProfile {
    int32_t frames;
    double stage_ms[GSR_PROFILE_STAGES]; /* summed over `frames` */
} GsrProfile;
int gsr_profile_enable(int mode);
int gsr_profile_collect(GsrProfile *out);

/*
 * Backward rasterization (upstream RasterizeGaussiansBackwardCUDA -> Rasterizer::backward).
 * `settings` / `in` are the forward's; the three state pointers are the buffers the forward filled (exact mode:
 * binning state carved for num_rendered instances).  Every gradient buffer is zeroed by the call.
 */
typedef struct GsrBackwardInputs {
    const float *dL_dout_color;    /* (3,H,W) */
    const float *dL_dout_invdepth; /* (1,H,W) or NULL */
    const int32_t *radii;          /* (P) from the forward */
    int64_t num_rendered;          /* R from the forward */
    const void *geom, *binning, *image;
} GsrBackwardInputs;

typedef struct GsrGrads {
    float *dL_dmeans2D;   /* (P,3)  pixel-NDC units, z unused */
    float *dL_dcolors;    /* (P,3) */
    float *dL_dopacity;   /* (P) */
    float *dL_dmeans3D;   /* (P,3) */
    float *dL_dcov3D;     /* (P,6) */
    float *dL_dsh;        /* (P,M,3) or NULL with colors_precomp */
    float *dL_dscales;    /* (P,3) or NULL with cov3D_precomp */
    float *dL_drots;      /* (P,4) or NULL with cov3D_precomp */
    float *dL_dconic;     /* unused (may be NULL): the compositor's per-Gaussian sums live in the geometry state */
    float *dL_dinvdepths; /* unused (may be NULL) */
    float *dL_dsh_rest;   /* (P,M-1,3) with GsrInputs.shs_rest (dL_dsh is then the (P,1,3) dc part), else NULL */
} GsrGrads;

int gsr_backward(const GsrSettings *settings, const GsrInputs *in, const GsrBackwardInputs *bw,
                 const GsrGrads *grads, void *stream);

/*
 * simple_knn._C.distCUDA2(points (P,3)) -> (P): mean of the squared distances to the 3 nearest OTHER points
 * (exact; self excluded by index, duplicates give 0).  `workspace` needs gsr_knn_workspace_bytes(P) bytes.
 */
size_t gsr_knn_workspace_bytes(int32_t P);
int gsr_knn_dist2(int32_t P, const float *points, float *mean_dist2, void *workspace, size_t workspace_bytes,
                  void *stream);

/*
 * fused_ssim_cuda.fusedssim / fusedssim_backward: images are (B,CH,H,W) contiguous; 11x11 Gaussian window
 * (sigma 1.5), zero "same" padding.  With train != 0 the three partial maps needed by the backward are stored.
 * The backward differentiates w.r.t. img1 only (as upstream).
 */
int gsr_ssim_forward(int32_t B, int32_t CH, int32_t H, int32_t W, float C1, float C2, const float *img1,
                     const float *img2, int32_t train, float *ssim_map, float *dm_dmu1, float *dm_dsigma1_sq,
                     float *dm_dsigma12, void *stream);
int gsr_ssim_backward(int32_t B, int32_t CH, int32_t H, int32_t W, float C1, float C2, const float *img1,
                      const float *img2, const float *dL_dmap, const float *dm_dmu1, const float *dm_dsigma1_sq,
                      const float *dm_dsigma12, float *dL_dimg1, void *stream);

/*
 * The photometric loss of the 3DGS training step, (1 - lambda) mean|x - t| + lambda (1 - mean ssim(x, t)) with
 * x = clamp(img, 0, 1) when clamp01 (what train.py builds from l1_loss, fused_ssim and render()'s clamp out of ~25
 * elementwise / reduction launches and their autograd), in three launches: the ssim forward pass with the sums folded
 * in, a one-workgroup sum in a fixed order (binary64), and -- gsr_photometric_loss_backward, after a forward with
 * keep_for_backward != 0 on the same scratch -- the ssim backward pass with the L1 sign term, the clamp mask and the
 * incoming gradient of the loss (grad_loss: one float on the device, NULL = 1) folded in.  img / target / dL_dimg:
 * (planes, H, W) float32; loss: one float on the device; dL_dimg = grad_loss x d loss / d img.  scratch:
 * gsr_photometric_loss_scratch_floats(planes, H, W) floats.
 * An extension (no upstream entry point); gsr_ssim_* above remain the drop-in for fused_ssim_cuda.
 */
size_t gsr_photometric_loss_scratch_floats(int32_t planes, int32_t H, int32_t W);
int gsr_photometric_loss(int32_t planes, int32_t H, int32_t W, const float *img, const float *target,
                         float lambda_dssim, int32_t clamp01, float *scratch, float *loss, int32_t keep_for_backward,
                         void *stream);
int gsr_photometric_loss_backward(int32_t planes, int32_t H, int32_t W, const float *img, const float *target,
                                  float lambda_dssim, int32_t clamp01, const float *scratch, const float *grad_loss,
                                  float *dL_dimg, void *stream);

/*
 * Fused per-step rigid transform of labelled Gaussians -- replaces GSWorld's per-link isin() mask / gather /
 * transform_gaussians / masked scatter passes (gs_world_wrapper.py:110-162,244-265; gs_utils.py:283-385) and the
 * full-model deepcopy with one pass.  label = (int)semantics[i]; k = lut[label] (or -1 / out of range: copy through);
 * transforms[k] = 17 floats: R row-major (9), t (3), uniform scale (1), quaternion of R as (w,x,y,z) (4).
 *   xyz' = R (scale * xyz) + t;   rot' = standardize(q_R (x) rot/|rot|) * |rot|.
 */
int gsr_transform_gaussians(int32_t P, const float *xyz, const float *rot, const float *semantics,
                            const int32_t *lut, int32_t lut_size, const float *transforms, int32_t K,
                            float *xyz_out, float *rot_out, void *stream);

/*
 * The same for E environments at once (gs_world_wrapper.py:239-242 renders `for i in range(num_envs)`, and
 * transform_gaussians returns (B,N,.) tensors for a batch of B poses): `transforms` is (E,K,17), the outputs are
 * (E,P,3) / (E,P,4), environment e under pose table e.  Optional scaling / scaling_out ((P,3) in, (E,P,3) out; both or
 * neither): the log-scale parameter of the parts flagged in `rescale` ((K) bytes, NULL = none) is rewritten the way the
 * reference rewrites it when it is given a per-environment scale vector (gs_utils.py: `inverse_sigmoid(exp(scaling) *
 * scale)` = log(x / (1 - x)), sic -- the tracked actors of the wrapper, gs_world_wrapper.py:146-157), copied otherwise.
 */
int gsr_transform_gaussians_batch(int32_t P, int32_t E, const float *xyz, const float *rot, const float *scaling,
                                  const float *semantics, const int32_t *lut, int32_t lut_size,
                                  const float *transforms, int32_t K, const uint8_t *rescale, float *xyz_out,
                                  float *rot_out, float *scaling_out, void *stream);

/*
 * Builds the 17-float transform table on the DEVICE from K row-major 4x4 rigid matrices (and optional uniform
 * scales, NULL = 1): the link / actor poses a GPU simulator already holds as device tensors
 * (gs_world_wrapper.py:118-120,146-156 compute them with torch on the simulation device).  The quaternion is
 * ManiSkill's matrix_to_quaternion (real part first, non-negative) in its float32 operation order.
 */
int gsr_pack_part_transforms(int32_t K, const float *matrices, const float *scales, float *table, void *stream);

/*
 * One closed-loop step's host values in ONE launch (gs_world_wrapper.py:110-162 computes the part poses per step, :238 the
 * cameras; a CPU simulator leaves both on the host): `src` is the DEVICE-VISIBLE address of pinned host memory
 * (gsr_pinned_device_address of a hipHostMalloc / torch pin_memory buffer), n floats; they are copied to `dst` (device),
 * and the K row-major 4x4 part matrices at src + mat_off (uniform scales at src + scale_off; scale_off < 0: all 1) are
 * packed into the 17-float pose table exactly as gsr_pack_part_transforms packs them.  Nothing but a kernel launch: the
 * call can be captured into a hipGraph, the step's host values then travel INSIDE the step's graph (no copy, no launch
 * between two replays).  The kernel reads the host buffer when it RUNS: keep it unchanged until then (a ring of slots).
 */
int gsr_pinned_device_address(const void *host, void **device);
int gsr_stage_step(int32_t n, const float *src, float *dst, int32_t K, int32_t mat_off, int32_t scale_off,
                   float *table, void *stream);

/* Self-test of the wave reductions used by the backward: out44[w] = sum(in256[64w .. 64w+63]) for the 4 waves, then
 * out44[4 + 10w + c] = sum over the wave's lanes l with l % (c + 2) == 0 of (c + 1) * in256[64w + l]  (ten different
 * per-lane values through the 10-component transpose-reduce). */
int gsr_selftest_wave_sum(const float *in256, float *out44, void *stream);

/* GSWorld's frame conversion (gs_world_wrapper.py:268-270): (3,H,W) float -> (H,W,3) uint8 with
 * (x*255).clamp(0,255) and a truncating cast.  `out` must be 4-byte aligned. */
int gsr_pack_rgb8(const float *color, int32_t width, int32_t height, uint8_t *out, void *stream);

/* upstream markVisible / checkFrustum: present[i] = p_view.z > near_plane. */
int gsr_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, float near_plane,
                     uint8_t *present, void *stream);

/*
 * Point clouds of rendered frames (pointcloud.hip: the full definition, evaluation order included, is its header comment).
 * Per environment e and camera c, from the depth / label maps of gsr_render_maps, the uint8 frame and the camera: a pixel
 * with depth > 0 unprojects to p = C2W (xv, yv, zv, 1) (C2W = the inverse of the view matrix, computed once per frame in
 * binary64), the output point is q = out_from_scene p, and the point is VALID when q lies in the crop box (if any) and its
 * label is not excluded (if a set is given).  Points are ordered camera by camera, then row-major by pixel.  A valid
 * point's slot holds xyzw = (q, 1), rgb and its label (-1 without label maps); any other slot xyzw = 0, rgb = 0, label -1.
 *   GSR_PC_DENSE:  N = sum over cameras of W H slots per environment, one per pixel; count[e] = valid points.
 *   GSR_PC_STRIDE: K slots; with n valid points and M = min(n, K), slot j < M holds the valid point of rank
 *                  floor(j n / M) (64-bit integers); count[e] = M.
 *   GSR_PC_FPS:    candidates as in STRIDE with M = min(n, fps_candidates); farthest-point sampling over them from
 *                  candidate 0 (squared distance ((dx dx) + (dy dy)) + dz dz in binary32, argmax with ties to the lowest
 *                  index); min(M, K) picks in pick order; count[e] = min(M, K).
 * Outputs: out_xyzw (E, N|K, 4) float32, out_rgb (E, N|K, 3) uint8, out_segmentation (E, N|K) int16, out_count (E) int32.
 * At most four launches on `stream`, no allocation, no synchronisation: the call can be captured into a hipGraph.  The
 * workspace (device, gsr_pointcloud_workspace bytes) holds per-workgroup counts and the FPS candidates.  Limits (else
 * GSR_E_INVALID): 1 <= E C <= GSR_PC_MAX_VIEWS; every environment's camera c has environment 0's size; at most
 * GSR_PC_MAX_VIEW_PIXELS pixels per view; 1 <= K <= GSR_PC_MAX_K; 1 <= fps_candidates <= GSR_PC_MAX_FPS_CANDIDATES; an
 * exclusion set needs every view's label map.
 */
#define GSR_PC_DENSE 0
#define GSR_PC_STRIDE 1
#define GSR_PC_FPS 2
#define GSR_PC_MAX_VIEWS 64
#define GSR_PC_MAX_K 8192
#define GSR_PC_MAX_FPS_CANDIDATES 16384
#define GSR_PC_MAX_VIEW_PIXELS (1 << 24)
typedef struct GsrCloudView {
    int32_t width, height;
    float tanfovx, tanfovy;         /* as the frame was rendered (GsrSettings) */
    const float *viewmatrix;        /* 16 floats: the frame's GsrInputs.viewmatrix (device-resident, read at run time) */
    const float *depth;             /* (H,W): gsr_render_maps out_depth */
    float depth_scale;              /* what that depth map was written with */
    const int16_t *label;           /* (H,W) gsr_render_maps out_label, or NULL */
    const uint8_t *rgb8;            /* (H,W,3) the frame, or NULL (rgb 0) */
} GsrCloudView;
typedef struct GsrCloudSpec {
    int32_t struct_size;            /* sizeof(GsrCloudSpec): the library rejects a mismatch (GSR_E_INVALID) */
    int32_t E, C;
    const GsrCloudView *views;      /* [host] E * C records, environment-major: view e * C + c */
    float out_from_scene[12];       /* [host] row-major 3 x 4 affine applied to every scene point */
    int32_t crop;                   /* 1: keep points with crop_lo <= q <= crop_hi (inclusive, per axis) */
    float crop_lo[3], crop_hi[3];
    const uint32_t *exclude;        /* 2048 words: bit (uint16)label set = drop the point; or NULL */
    int32_t mode, K, fps_candidates;
    float *out_xyzw;
    uint8_t *out_rgb;
    int16_t *out_segmentation;
    int32_t *out_count;
    void *workspace;
    int64_t workspace_bytes;
} GsrCloudSpec;
int gsr_pointcloud_workspace(const GsrCloudSpec *spec, int64_t *bytes);
int gsr_render_pointcloud(const GsrCloudSpec *spec, void *stream);

/*
 * Cameras from simulator sensor poses (camera.hip: the full definition, evaluation order included, is its header comment).
 * Per view k < n: the OpenCV world->camera extrinsic E = [A | t] of the simulator (ManiSkill get_sensor_params()
 * extrinsic_cv) becomes the 36-float camera record the frames read -- world_view (16, = W2C^T) | full_proj (16) |
 * centre (3) | pad (1, written 0) -- of the 3DGS camera GSWorld builds from it (gs_world_wrapper.py cam_maniskill2gs): the
 * simulator camera placed at scale_sim2real x its position, left-multiplied by rigid_sim2real.  Binary64 throughout,
 * rounded to binary32 once per output.  `projection` holds each view's getProjectionMatrix(0.01, 100, FoVx, FoVy)^T as
 * float32 (fixed for a camera's lifetime).  View k reads extrinsic + offsets[3k] (12 floats, row-major 3 x 4),
 * projection + offsets[3k + 1] (16 floats) and writes out + offsets[3k + 2] (36 floats); offsets NULL: 12 k, 16 k, 36 k.
 * Offsets are not checked against any buffer (device memory): the caller owns them.  Extrinsics are read when the kernel
 * runs.  One launch on `stream`, no allocation, no synchronisation: the call can be captured into a hipGraph.  Limits
 * (else GSR_E_INVALID): struct_size, 1 <= n <= GSR_CAM_MAX_VIEWS, non-null extrinsic / projection / out, a finite
 * non-zero scale_sim2real.
 */
#define GSR_CAM_MAX_VIEWS 4096
#define GSR_CAM_RECORD_FLOATS 36
typedef struct GsrSensorCameras {
    int32_t struct_size;            /* sizeof(GsrSensorCameras): the library rejects a mismatch (GSR_E_INVALID) */
    int32_t n;                      /* views */
    const float *extrinsic;         /* (3,4) row-major world->camera matrices, float32 */
    const float *projection;        /* 16 floats per view: the projection matrix transposed, row-major */
    float *out;                     /* 36-float records */
    const int32_t *offsets;         /* 3 n float offsets (extrinsic, projection, record) per view, or NULL (packed) */
    double rigid_sim2real[16];      /* [host] row-major 4 x 4 */
    double scale_sim2real;          /* [host] */
} GsrSensorCameras;
int gsr_cameras_from_extrinsics(const GsrSensorCameras *spec, void *stream);

/*
 * The optimizer step of a training iteration (optim.hip): Adam on the Gaussians a frame saw, for up to
 * GSR_ADAM_MAX_GROUPS parameter tensors in ONE launch.  This comment is the definition.  Group k holds N Gaussians of M
 * floats each: param, grad, exp_avg (m), exp_avg_sq (v), all (N, M) contiguous float32 on the device.  For every element
 * of a VISIBLE Gaussian, in binary32, every operation rounded once, nothing contracted, (1 - beta) formed once in
 * binary32 on the host:
 *     m' = (beta1 * m) + ((1 - beta1) * g)
 *     v' = (beta2 * v) + (((1 - beta2) * g) * g)
 *     p' = p + (((-lr) * m') / (sqrtf(v') + eps))
 * with `/` and sqrtf the correctly rounded ones and denormals kept; m', v', p' are stored.  There is no bias correction
 * and no step counter (the 3DGS sparse optimizer's semantics).  A non-finite gradient of a visible Gaussian propagates
 * as the arithmetic says.  An INVISIBLE Gaussian's param, exp_avg and exp_avg_sq keep their bits -- its moments do not
 * decay: this is not dense Adam -- and its grad is never read (it may hold anything, NaN included).  Visibility is per
 * Gaussian and shared by the groups: `visible` NULL with GSR_VISIBLE_ALL, N uint8 / bool with GSR_VISIBLE_MASK8 (!= 0),
 * N int32 with GSR_VISIBLE_RADII (> 0: the `radii` a forward wrote, as they are).
 * Pointers need only be 4-byte aligned: a group whose four arrays are all 16-byte aligned is walked in 16-byte vectors
 * (one that straddles Gaussians of different visibility updates exactly the visible one's elements), any other group
 * element by element; the result is the same.  Element indices are 64-bit.  One launch on `stream`, no allocation, no
 * synchronisation: the call can be captured into a hipGraph, and a replay repeats the captured lr.
 * N == 0 returns GSR_OK without touching the device.  GSR_E_INVALID: struct_size, N < 0, num_groups outside
 * 1..GSR_ADAM_MAX_GROUPS, an M outside 1..4096, a null pointer in a used group when N > 0, an unknown visible_kind, a
 * kind that does not match `visible` being NULL or not.
 */
#define GSR_ADAM_MAX_GROUPS 8
#define GSR_VISIBLE_ALL 0   /* visible == NULL: every Gaussian */
#define GSR_VISIBLE_MASK8 1 /* uint8 / bool (N): != 0 */
#define GSR_VISIBLE_RADII 2 /* int32 (N): > 0 -- the forward's radii as they are */
typedef struct GsrAdamGroup {
    float *param;                /* (N, M) contiguous float32, device -- as are the next three */
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int32_t M;                   /* floats per Gaussian, 1 <= M <= 4096 */
    float lr, beta1, beta2, eps; /* [host] */
} GsrAdamGroup;
typedef struct GsrAdamStep {
    int32_t struct_size;         /* sizeof(GsrAdamStep): the library rejects a mismatch (GSR_E_INVALID) */
    int32_t N;                   /* Gaussians */
    int32_t num_groups;          /* groups[0 .. num_groups) are used */
    int32_t visible_kind;        /* GSR_VISIBLE_* */
    const void *visible;
    GsrAdamGroup groups[GSR_ADAM_MAX_GROUPS];
} GsrAdamStep;
int gsr_adam_update(const GsrAdamStep *step, void *stream);

/*
 * The densification statistics of a training iteration (optim.hip), upstream's `max_radii2D[vis] = max(...)` and
 * `add_densification_stats` without the compaction and host read of `(radii > 0).nonzero()`.  For every Gaussian with
 * radii[i] > 0 -- the others are untouched --, with (gx, gy) = grad_means2D[3 i], grad_means2D[3 i + 1] (the third column
 * is never read), in binary32, every operation rounded once:
 *     grad_accum[i]  = grad_accum[i] + sqrtf((gx * gx) + (gy * gy))
 *     denom[i]       = denom[i] + 1
 *     max_radii2D[i] = fmaxf(max_radii2D[i], (float)radii[i])          (when max_radii2D is not NULL)
 * One launch on `stream`, no allocation, no synchronisation (capturable).  N == 0 returns GSR_OK without touching the
 * device; GSR_E_INVALID: N < 0, or a null radii / grad_means2D / grad_accum / denom when N > 0.
 */
int gsr_densification_stats(int32_t N, const int32_t *radii, const float *grad_means2D /* (N,3) */,
                            float *grad_accum /* (N) */, float *denom /* (N) */,
                            float *max_radii2D /* (N) or NULL */, void *stream);

/*
 * Densify-and-prune of the model on the device (densify.hip): what upstream's densify_and_prune does every
 * densification_interval iterations -- densify_and_clone, densify_and_split (N = 2), the final prune_points -- as two
 * calls, so that the data-dependent output size crosses to the host exactly once, between them.  This comment is the
 * definition.
 *
 * gsr_densify_plan decides.  Per Gaussian i < N, in binary32, every operation rounded once, nothing contracted, expf /
 * logf the accurate (<= 1 ulp) ones, s = scaling[3 i ..] (log space), o = opacity[i] (logit):
 *     g          = grad_accum[i] / denom[i];  a NaN g becomes 0
 *     hot_clone  = fabsf(g) >= grad_threshold;       hot_split = g >= grad_threshold
 *     smax       = max(max(expf(s0), expf(s1)), expf(s2)), a max that PROPAGATES NaN (torch.max, not fmaxf)
 *     small      = smax <= dense_limit               (dense_limit = percent_dense * extent, formed by the caller)
 *     clone_sel  = hot_clone && small;               split_sel = hot_split && !small
 *     op         = 1 / (1 + expf(-o));               prune_op = op < min_opacity
 *     big_self   = prune_world_size && smax > world_limit          (world_limit = 0.1f * extent, from the caller)
 *     child_s[k] = logf(expf(s[k]) / 1.6f)
 *     big_child  = prune_world_size && max_k expf(child_s[k]) > world_limit      (the same NaN-propagating max)
 *     self kept          iff !split_sel && !prune_op && !big_self
 *     a clone emitted    iff  clone_sel && !prune_op && !big_self
 *     two children emitted iff split_sel && !prune_op && !big_child
 * (upstream's screen-size test is absent on purpose: densification_postfix zeroes max_radii2D before the final prune
 * reads it, so inside this sequence it never selects anything.)  The output rows are upstream's order, four segments,
 * each ascending in i: kept selves | clones | first children | second children.  counts[4] (device int32) receives
 * kept, clones, split parents whose children are emitted, N_out = kept + clones + 2 split; `workspace`
 * (gsr_densify_workspace_bytes(N) bytes, 16-byte aligned) receives what gsr_densify_apply needs.  Three launches on
 * `stream`, no allocation, no synchronisation.  N == 0 returns GSR_OK without touching the device (counts is not written).
 * GSR_E_INVALID: struct_size, N < 0 or N > 2^30, a null pointer, a workspace that is too small or misaligned.
 *
 * gsr_densify_apply moves the data: ONE launch for up to GSR_ADAM_MAX_GROUPS groups.  Group k has sources param,
 * exp_avg, exp_avg_sq (N, M) and destinations out_* (N_out, M), contiguous float32; the four moment pointers are all
 * given or all NULL (a group that never stepped).  Output row r with parent i (r's segment decides its kind):
 *     kept self:  param, exp_avg, exp_avg_sq of row i, bit for bit
 *     clone:      param of row i bit for bit, zero moments
 *     child c (0 first, 1 second): zero moments; param of row i bit for bit, except
 *         role GSR_DENSIFY_SCALING:  child_s[k] above
 *         role GSR_DENSIFY_XYZ:      ((R_k0 v0 + R_k1 v1) + R_k2 v2) + xyz[i][k],  v[j] = expf(s[j]) * noise[i][c][j]
 * with R the rotation matrix of the raw quaternion q = rotation[4 i ..] = (r, x, y, z), as the 3DGS python layer's
 * build_rotation forms it: n = sqrtf(((r r + x x) + y y) + z z), each component divided by n, then
 *     R00 = 1 - 2 (y y + z z)   R01 = 2 (x y - r z)       R02 = 2 (x z + r y)
 *     R10 = 2 (x y + r z)       R11 = 1 - 2 (x x + z z)   R12 = 2 (y z - r x)
 *     R20 = 2 (x z - r y)       R21 = 2 (y z + r x)       R22 = 1 - 2 (x x + y y)
 * `xyz`, `scaling`, `rotation` are the model's raw tensors (the XYZ / SCALING groups' params, as a rule); `noise` is
 * (N, 2, 3) standard normals INDEXED BY PARENT, so it can be drawn before the number of splits is known.  `parent`
 * (int32, N_out) always receives i for every row.  N and the workspace are those of the plan; N_out is what the caller
 * read from counts[3] -- rows past the plan's own N_out are not written.  Pointers need only be 4-byte aligned: a group
 * whose destinations are all 16-byte aligned is written in 16-byte vectors.  Gaussian indices are 32-bit, element
 * indices 64-bit.  No allocation, no synchronisation.  N == 0 and N_out == 0 return GSR_OK without a launch.
 * GSR_E_INVALID: struct_size, N outside 0..2^30, N_out outside 0..2 N, num_groups outside 0..GSR_ADAM_MAX_GROUPS, an M
 * outside 1..4096 (the XYZ and SCALING roles: M = 3), an unknown role, a null pointer, moments given in part, a
 * workspace too small or misaligned, an output that overlaps an input, the workspace or another output.
 */
#define GSR_DENSIFY_COPY 0
#define GSR_DENSIFY_XYZ 1
#define GSR_DENSIFY_SCALING 2
typedef struct GsrDensifyPlan {
    int32_t struct_size;         /* sizeof(GsrDensifyPlan): the library rejects a mismatch (GSR_E_INVALID) */
    int32_t N;                   /* Gaussians */
    const float *grad_accum;     /* (N) -- device, as are denom, scaling, opacity */
    const float *denom;          /* (N) */
    const float *scaling;        /* (N, 3) raw (log) */
    const float *opacity;        /* (N) raw (logit) */
    float grad_threshold;        /* [host] */
    float min_opacity;           /* [host] */
    float dense_limit;           /* [host] percent_dense * extent */
    float world_limit;           /* [host] 0.1f * extent */
    int32_t prune_world_size;    /* upstream's `if max_screen_size:` */
    int32_t reserved;
    int32_t *counts;             /* device int32[4]: kept, clones, split, N_out */
    void *workspace;
    int64_t workspace_bytes;
} GsrDensifyPlan;
typedef struct GsrDensifyGroup {
    const float *param;          /* (N, M) */
    const float *exp_avg;        /* (N, M) or NULL */
    const float *exp_avg_sq;
    float *out_param;            /* (N_out, M) */
    float *out_exp_avg;          /* (N_out, M) or NULL */
    float *out_exp_avg_sq;
    int32_t M;                   /* floats per Gaussian, 1 <= M <= 4096 */
    int32_t role;                /* GSR_DENSIFY_* */
} GsrDensifyGroup;
typedef struct GsrDensifyApply {
    int32_t struct_size;         /* sizeof(GsrDensifyApply) */
    int32_t N;                   /* the plan's N */
    int32_t N_out;               /* counts[3], as the caller read it */
    int32_t num_groups;
    const void *workspace;       /* the plan's */
    int64_t workspace_bytes;
    const float *xyz;            /* (N, 3) */
    const float *scaling;        /* (N, 3) raw */
    const float *rotation;       /* (N, 4) raw */
    const float *noise;          /* (N, 2, 3) */
    int32_t *parent;             /* (N_out) */
    GsrDensifyGroup groups[GSR_ADAM_MAX_GROUPS];
} GsrDensifyApply;
int64_t gsr_densify_workspace_bytes(int32_t N); /* [host] multiple of 256 */
int gsr_densify_plan(const GsrDensifyPlan *plan, void *stream);
int gsr_densify_apply(const GsrDensifyApply *apply, void *stream);

/*
 * Nearest point of a reference cloud for every point of a query cloud (nnquery.hip), and the two real2sim steps that rest
 * on it: label transfer with bounding-box validation (GSWorld real2sim_utils/segment_utils.py) and the sums of one
 * point-to-point ICP iteration with scaling (real2sim/scripts/icp.py).  This comment is the definition.
 *
 * gsr_nn_build builds the search structure of `ref` (n_ref, 3) float32 once, into caller-owned `index_mem` of
 * gsr_nn_index_bytes(n_ref) bytes (256-byte aligned): the points in Morton order (30-bit codes in the cloud's own bounds),
 * their sorted codes, the permutation back to the caller's numbering and its inverse, the bounds, and the AABBs of boxes of
 * 1024 consecutive sorted points.  `ref` is not needed afterwards.  Coordinates must be finite (not checked here).
 * n_ref == 0 is legal and launches nothing.  No allocation, no synchronisation.
 *
 * gsr_nn_query: for every query i < n_query, with x' the query itself or, when use_transform, row r of it
 *     x'[r] = fmaf(m[r][2], z, fmaf(m[r][1], y, m[r][0] * x)) + m[r][3]          (m = query_transform, row-major 3 x 4)
 * and d2(j) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), d = x' - ref[j], all in binary32:
 *     index[i] = the j that minimises d2(j), the LOWEST such j on ties;  dist2[i] = that d2
 *     index[i] = -1, dist2[i] = +inf  when n_ref == 0, when a coordinate of x' is not finite, or when max_dist2 >= 0 and
 *                                     the minimum exceeds it (d2 == max_dist2 is still a match)
 * `query_out` (n_query, 3), when not NULL, receives x'.  The answer is exact -- it is the O(n m) definition whatever the
 * launch shape or the order of the queries.  `workspace`: gsr_nn_query_workspace_bytes(n_query) bytes, 256-byte aligned.
 * n_query == 0 returns GSR_OK without a launch.  No allocation, no synchronisation.
 * GSR_E_INVALID: struct_size, a negative size, a null pointer that is needed, a NaN max_dist2, memory too small or misaligned.
 */
size_t gsr_nn_index_bytes(int32_t n_ref);            /* [host] multiple of 256, monotone in n_ref */
int gsr_nn_build(int32_t n_ref, const float *ref, void *index_mem, size_t index_bytes, void *stream);
typedef struct GsrNnQuery {
    int32_t struct_size;         /* sizeof(GsrNnQuery) */
    int32_t n_ref;               /* the n_ref index_mem was built for */
    const void *index_mem;       /* what gsr_nn_build wrote (may be NULL when n_ref == 0) */
    int64_t index_bytes;
    int32_t n_query;
    int32_t use_transform;       /* 0: query_transform is not read */
    const float *query;          /* (n_query, 3) -- device */
    float query_transform[12];   /* [host] row-major 3 x 4 */
    float max_dist2;             /* [host] negative: no limit (-0 is the limit 0) */
    int32_t reserved;
    int32_t *index;              /* (n_query) out */
    float *dist2;                /* (n_query) out */
    float *query_out;            /* (n_query, 3) out, or NULL */
    void *workspace;
    int64_t workspace_bytes;
} GsrNnQuery;
size_t gsr_nn_query_workspace_bytes(int32_t n_query); /* [host] multiple of 256, monotone in n_query */
int gsr_nn_query(const GsrNnQuery *query, void *stream);

/*
 * gsr_label_transfer restates transfer_labels_with_bbox's validation loop per point i < n, with p = points[i] (the
 * query's query_out), j = index[i], and the box table's rows in the caller's order (row k: box_labels[k], box_bounds[k] =
 * min xyz, max xyz).  The squared distance to a box is
 *     e[c] = fmaxf(fmaxf(min[c] - p[c], 0), p[c] - max[c]);   b2 = fmaf(e2, e2, fmaf(e1, e1, e0 * e0))
 * and t2 = threshold * threshold, both in binary32:
 *     L = -1 when j < 0 or j >= n_ref, else ref_labels[j]
 *     L == -1                         -> labels[i] = -1
 *     no row carries L                -> labels[i] = -1
 *     b2(first row that carries L) <= t2 -> labels[i] = L
 *     otherwise                       -> the label of the row with the smallest b2 among rows with b2 <= t2 (strict <
 *                                        in row order: the first row wins a tie), or -1 when no row qualifies
 * One launch, one thread per point, the table in LDS.  n == 0 returns GSR_OK without a launch.
 * GSR_E_INVALID: struct_size, n < 0, n_boxes outside 0..GSR_LABEL_MAX_BOXES, a null pointer that is needed.
 */
#define GSR_LABEL_MAX_BOXES 1024
typedef struct GsrLabelTransfer {
    int32_t struct_size;         /* sizeof(GsrLabelTransfer) */
    int32_t n;
    const int32_t *index;        /* (n) from gsr_nn_query */
    const float *points;         /* (n, 3) the transformed queries */
    const int32_t *ref_labels;   /* (n_ref) */
    int32_t n_ref;
    int32_t n_boxes;
    const int32_t *box_labels;   /* (n_boxes) -- device */
    const float *box_bounds;     /* (n_boxes, 6) -- device */
    float threshold;             /* [host] */
    int32_t reserved;
    int32_t *labels;             /* (n) out */
} GsrLabelTransfer;
int gsr_label_transfer(const GsrLabelTransfer *transfer, void *stream);

/*
 * gsr_icp_moments: the sums one Umeyama update needs, in binary64, over the inliers i (0 <= index[i] < n_ref) of a
 * query of the transformed sources: p' = the transform of source[i] as gsr_nn_query forms it (binary32, then widened),
 * q = the reference point index[i] of the built structure.  sums[18] (device doubles):
 *     [0] count   [1..3] sum p'   [4..6] sum q   [7..15] sum p'[r] q[c] at 7 + 3 r + c   [16] sum |p'|^2   [17] sum dist2[i]
 * Per-workgroup partial sums in a fixed order, then one workgroup adds them in a fixed order: no floating atomics, two
 * calls give the same bytes.  `workspace`: GSR_ICP_WORKSPACE_BYTES bytes, 8-byte aligned.  n == 0 or n_ref == 0 writes zeros.
 * GSR_E_INVALID: struct_size, a negative size, a null pointer that is needed, a workspace too small or misaligned.
 */
#define GSR_ICP_WORKSPACE_BYTES (256 * 18 * 8)
typedef struct GsrIcpMoments {
    int32_t struct_size;         /* sizeof(GsrIcpMoments) */
    int32_t n;                   /* source points */
    const float *source;         /* (n, 3) */
    float transform[12];         /* [host] row-major 3 x 4 */
    int32_t use_transform;
    int32_t n_ref;
    const void *index_mem;       /* the structure the query ran against */
    int64_t index_bytes;
    const int32_t *index;        /* (n) */
    const float *dist2;          /* (n) */
    double *sums;                /* (18) out */
    void *workspace;
    int64_t workspace_bytes;
} GsrIcpMoments;
int gsr_icp_moments(const GsrIcpMoments *moments, void *stream);

/*
 * gsr_train_loss / gsr_train_loss_backward: the whole loss of a 3DGS training iteration (upstream train.py with
 * train_test_exp, an alpha mask and the inverse-depth regularisation) and its gradients, three launches each way.
 * All device arrays are float32.  With E = exposure (row-major 3 x 4), per pixel and in this order of operations:
 *     y_c = ((color_0 E[0][c] + color_1 E[1][c]) + color_2 E[2][c]) + E[c][3]      (exposure == NULL: y = color)
 *     x_c = clamp(y_c, 0, 1)   (a NaN stays a NaN);    alpha_mask != NULL: x_c = x_c * alpha
 *     loss = (1 - lambda) mean|x - target| + lambda (1 - mean ssim(x, target))      (the sums of gsr_photometric_loss)
 *     depth group present: loss += depth_weight * mean over H W of |(invdepth - mono_invdepth) * depth_mask|
 * Every sum over pixels is per-workgroup partial sums in a fixed order (binary32), then one workgroup adds them in a fixed
 * order in binary64: no floating atomics, two calls give the same bits.  Without exposure, alpha mask and depth group the
 * value and dL_dcolor are those of gsr_photometric_loss(clamp01 = 1), bit for bit.
 * terms (4 floats, or NULL): total, mean|x - target|, mean ssim, the unweighted depth mean (0 without the group).
 * gsr_train_loss_backward -- after a gsr_train_loss with keep_for_backward != 0 on the same scratch and the same inputs --
 * writes, all scaled by grad_loss (one float on the device, NULL = 1):
 *     dL_dcolor (3,H,W);  dL_dinvdepth (H,W) when the depth group is present;  dL_dexposure (12) when exposure is.
 * sign(0) = 0; the clamp passes the gradient where 0 <= y <= 1 (bounds included) and stops it outside, towards color and
 * towards E alike.  dL_dexposure[4 i + c] = sum color_i g_c (i, c < 3), dL_dexposure[4 c + 3] = sum g_c, g = dL/dy.
 * scratch: 8-byte aligned; gsr_train_loss_scratch_floats(H, W) floats suffice for every call of that size (0 for an invalid
 * size), gsr_train_loss_scratch_needed(loss) is what THIS call needs -- the same arithmetic on the host, from H, W and which of
 * exposure / alpha_mask are present (without both, a third less) -- and what scratch_floats is checked against; forward and
 * backward of one call agree on it.
 * GSR_E_INVALID (before any device work): struct_size, H or W < 1 or H W > 2^28, a null color / target / scratch / loss,
 * a depth group of which only a part is present, a non-finite lambda_dssim or depth_weight, scratch_floats too small,
 * a scratch that is not 8-byte aligned, and in the backward a missing dL_dcolor, dL_dinvdepth (depth group) or dL_dexposure (exposure).
 */
typedef struct GsrTrainLoss {
    int32_t struct_size;         /* sizeof(GsrTrainLoss) */
    int32_t H, W;
    float lambda_dssim;          /* [host] */
    const float *color;          /* (3,H,W) the rasterizer's out_color, before exposure and clamp */
    const float *target;         /* (3,H,W) */
    const float *exposure;       /* (12) or NULL */
    const float *alpha_mask;     /* (H,W) or NULL */
    const float *invdepth;       /* (H,W) the rasterizer's out_invdepth -- depth group: all three or none */
    const float *mono_invdepth;  /* (H,W) */
    const float *depth_mask;     /* (H,W) */
    float depth_weight;          /* [host] */
    int32_t keep_for_backward;
    float *scratch;
    int64_t scratch_floats;
    float *loss;                 /* (1) out */
    float *terms;                /* (4) out, or NULL */
    const float *grad_loss;      /* backward: (1) or NULL = 1 */
    float *dL_dcolor;            /* backward: (3,H,W) out */
    float *dL_dinvdepth;         /* backward: (H,W) out (depth group) */
    float *dL_dexposure;         /* backward: (12) out (exposure) */
} GsrTrainLoss;
size_t gsr_train_loss_scratch_floats(int32_t H, int32_t W);
size_t gsr_train_loss_scratch_needed(const GsrTrainLoss *loss);
int gsr_train_loss(const GsrTrainLoss *loss, void *stream);
int gsr_train_loss_backward(const GsrTrainLoss *loss, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
