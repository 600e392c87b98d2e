/*
 * vpho_hip.h -- C ABI of the MI355X (gfx950) kernels behind vpho_amd's `vpho_net.forward(mode='predict')`.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`; nothing is owned or freed by the library
 *     (outputs are caller-allocated), no torch types appear in any signature;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises unless stated;
 *   - return value: 0 on success, non-zero on error with a message retrievable by vpho_last_error();
 *   - activations are fp32 NHWC ("pixel-major, channel-minor"); row-major matrices otherwise;
 *   - thread-compatible (one caller per stream), not re-entrant on the same output buffers.
 *
 * Each entry point names the reference call site (file:line under zhoujun-7/VPHO) whose arithmetic it replaces.
 */
#ifndef VPHO_HIP_H
#define VPHO_HIP_H

/* The library is built with -fvisibility=hidden: the entry points declared here are its ONLY exported symbols
 * (tests/test_abi.py compares `nm -D` with this header). */
#if defined(__GNUC__) || defined(__clang__)
#define VPHO_API __attribute__((visibility("default")))
#else
#define VPHO_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

VPHO_API const char* vpho_last_error(void);
VPHO_API int vpho_abi_version(void);   /* 14 */

/* Opt-in timing of one kernel class with HIP events recorded on the launch stream around every launch
 * (0 = conv_igemm 128x128 tile, 1 = conv_igemm 64x64 tile, 2 = fused score head, 3 = conv_igemm 128x64 tile; HBM-bound kernels,
 * reported in bytes: 4 = MANO FK, 5 = object physics score, 6 = hand cascade fuse, 7 = RoIAlign, 8 = bilinear resize; 9 = Winograd
 * convolution, 10 / 11 = weight-gradient TN GEMM with 64x64 / 128x128 tiles, 12 = pseudo-force optimiser, 13 = pose encoder).
 * vpho_prof_collect waits for the recorded events and returns the summed kernel time, the launch count, the algorithmic
 * flop (2*M*N*K) and the algorithmic bytes (operands once) issued. */
VPHO_API int vpho_prof_enable(int kernel_class, int on);
VPHO_API int vpho_prof_collect(int kernel_class, double* total_ms, long long* launches, double* total_flops, double* total_bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Convolution / linear layers as one implicit-GEMM kernel on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces every nn.Conv2d + BatchNorm(eval) + LeakyReLU/ReLU (+ residual add) group of
 *   lib/model/backbone_FPN_HFL.py:70-109,326-350, head_inplane.py:102-107, encoding.py:21-36,58-73,
 *   cross_module.py:126-127 and every nn.Linear of head_mano.py:61-70, physics.py:700-712, cross_module.py:104-134,
 *   denoiser.py:68-76 (a Linear is the 1x1 case with H=W=1).
 * y[n,oy,ox,co] = act( sum_{r,s,c} pre(x[n, oy*stride-pad_y+r, ox*stride-pad_x+s, c]) * w[co][(r*KW+s)*Cin+c]
 *                      + bias[co] + res[n,oy,ox,co] ),  act(v) = v>0 ? v : v*out_slope
 * pre(v) = lrelu(v*in_scale[c]+in_shift[c], in_slope) when in_scale != NULL (pre-activation BN of encoding.Residual),
 * zero padding is applied after pre().  BatchNorm following a conv is folded into w/bias by the caller.
 * Requirements: Cin % 4 == 0, x_ld % 4 == 0 (x_ld = floats between consecutive pixels of x), 16-byte aligned x and w.
 * The same kernel is the GEMM of the training slices (H=W=1: rows x Cin times Cout x Cin transposed).
 */
typedef struct {
    const float* x; const float* w; const float* bias;
    const float* in_scale; const float* in_shift;
    const float* res; float* y;
    int N, H, W, Cin, x_ld;
    int Cout, KH, KW, stride, pad_y, pad_x, OH, OW;
    long long y_sn, y_sy, y_sx;      /* element strides of y for (n, oy, ox); channel stride is 1 */
    long long r_sn, r_sy, r_sx;      /* same for res */
    float in_slope, out_slope;
    /* Optional (zero = off).  w_ld: floats between consecutive rows of w when a launch reduces only a K-slice of wider rows.
     * splits > 1: blockIdx.y = 0..splits-1 runs the same problem on x + i*x_split, w + i*w_split and writes y + i*y_split --
     * partial sums of a long reduction (the pixel dimension of a weight gradient) for the caller to add; no bias / res. */
    int w_ld, splits;
    long long x_split, w_split, y_split;
    /* Optional (NULL = off; ABI version 4): y = gate > 0 ? y : y * gate_slope after the epilogue, `gate` laid out like y (same
     * strides, pointing at the element that corresponds to y[0]) -- the backward of a LeakyReLU given its output, fused into the
     * input-gradient convolution (torch autograd of nn.LeakyReLU in Bottleneck / Residual, backbone_FPN_HFL.py:326, encoding.py:21-36). */
    const float* gate;
    float gate_slope;
    /* Optional (NULL = off; ABI version 5): compute only the output pixels listed in row_map[0 .. *row_count) -- each entry the
     * linear index (n*OH + oy)*OW + ox of an output pixel -- and write them as the rows of a COMPACT (*row_count, Cout) matrix
     * (y_sx = floats between rows; y_sn / y_sy unused; res, if given, is compact too).  Both live on the device: the grid is
     * sized for all N*OH*OW pixels and tiles beyond *row_count exit, so the launch needs no host round trip and replays in a
     * HIP graph with new windows.  Used for the FPN smoothing convolutions, whose maps are read only through RoIAlign
     * (VPHO.py:126-129): see vpho_roi_windows_i32.  rows_hint (0 = unknown) only feeds the profiling counters. */
    const int* row_map;
    const int* row_count;
    int rows_hint;
    int rows_scatter;                /* 1: keep y's (n, oy, ox) layout and write only the listed pixels (the rest of y is untouched) */
    /* Optional, opt-in (NULL / 0 = fp32 MFMA, the default and the path parity is stated on): w as three bf16 planes [3][Cout][K]
     * with w = plane0 + plane1 + plane2 exactly, plane_terms = 6 or 9 bf16 products per fp32 product, fp32 accumulation.  Taken for
     * Cin % 16 == 0, no prologue affine, no splits / gate, 16-byte addressable output rows; other shapes run the fp32 kernels. */
    const void* w_planes;
    int plane_terms;
    /* Optional (NULL = off; ABI version 8): the residual is a COARSER map, added after bilinear up-sampling to the output grid --
     * y = act(conv + bias + F.interpolate(res_up, size=(OH, OW), mode='bilinear', align_corners=False)[n, oy, ox, co]) -- the FPN's
     * top-down step `_upsample_add(p, lateral(c))` (backbone_FPN_HFL.py:66-68,98-104) inside the lateral 1x1 convolution's epilogue:
     * the finer map is written once instead of written, re-read and re-written by a separate pass.  res_up: (N, ru_H, ru_W, ru_ld)
     * NHWC, ru_ld % 4 == 0, 16-byte aligned; exclusive with `res`; the same arithmetic, in the same order, as
     * vpho_resize_bilinear_nhwc_f32(accumulate = 1) after the convolution: bit-identical.  Works with row_map / rows_scatter. */
    const float* res_up;
    int ru_H, ru_W, ru_ld;
    /* Optional (NULL = off; ABI version 8): a SECOND input of a 1x1 convolution, concatenated behind x along the channel axis without a
     * copy: y = act(w[:, :Cin] . x[n, oy*stride, ox*stride, :] + w[:, Cin:] . x2[n, oy*stride2, ox*stride2, :] + bias (+ res)), w packed as
     * [Cout][Cin + Cin2].  It merges the projection shortcut of a ResNet stage's first bottleneck (downsample.0/1: a 1x1 convolution +
     * BatchNorm of the block input, stride 1 or 2, backbone_FPN_HFL.py:311-350) into conv3: one launch, and the 4C-wide shortcut map is
     * neither written nor re-read.  x2: (N, H2, W2, x2_ld) NHWC; needs KH = KW = 1, no padding, Cin % 32 == 0, Cin2 % 32 == 0, no pixel
     * list / prologue / splits.  The sum over the Cin + Cin2 products is one accumulation chain: results differ from the two-launch
     * form (sum, bias, add) by fp32 rounding. */
    const float* x2;
    int Cin2, x2_ld, stride2, H2, W2;
    /* Optional (0 / 1 = off; ABI version 11): GROUPED launch -- group g = 0 .. groups-1 runs the same problem on x + g*x_group, w + g*w_group,
     * bias + g*bias_group, y + g*y_group, res + g*res_group, x2 + g*x2_group, in_scale / in_shift + g*pre_group, res_up + g*ru_group (floats;
     * multiples of 4; x_group = 0: every group reads the same input).  The hand and the object branch of the feature path are twins
     * -- layer2 / layer3, FPN laterals, heat-map heads, encoders: same shapes, different weights (backbone_FPN_HFL.py:79-109, VPHO.py:131-149)
     * -- and run as ONE launch each: twice the tiles, half the launches; every output element's k order is unchanged (bit-identical to
     * the two single launches).  No splits / pixel list / gate / bf16 planes. */
    int groups;
    long long x_group, w_group, bias_group, y_group, res_group, x2_group, pre_group, ru_group;
    /* Optional (NULL = off; ABI version 12, partial-row layout 13): the reductions of a train-mode BatchNorm next to this convolution, taken in its epilogue
     * while the output tile is still on the chip (nn.BatchNorm2d under model.train() behind every convolution of Bottleneck / Residual /
     * HeadHeatmap2: backbone_FPN_HFL.py:330-350, encoding.py:21-36, head_inplane.py:40-58; train_diff_hand_obj.py:171,181).
     *   stats      device, [stats_cap][6][Cout] floats: row t = the partial sums over the output rows of M-tile t of the values v this
     *              launch STORES (after bias / residual / activation / gate): plane 0 = sum v, plane 1 = sum v * v (fp32, as in ABI 12),
     *              and about a pivot p = the tile's first value of the channel: plane 2 = p, plane 3 = sum (v - p), plane 4 =
     *              sum (v - p)^2, plane 5 = the number of rows -- the statistics pass of
     *              the BatchNorm that FOLLOWS the convolution (vpho_bn_train_forward_stats_f32 merges planes 2 .. 5 in fp64).  Centred sums: the
     *              variance of a channel whose |mean| is far above its std does not come from E[v^2] - mean^2 of rounded sums.  Plain
     *              stores, one writer per element, fixed order: bit-reproducible.
     *   stats_rows HOST pointer, written before the call returns: the number of partial rows the launch writes (= its M-tiles), or 0 when
     *              the kernel chosen for this shape does not produce them (the caller then runs the stand-alone reduction).  A launch that
     *              needs more than stats_cap rows writes none and reports 0.
     *   bn_x != NULL (input-gradient convolutions): the launch's output is the gradient at the OUTPUT of act(BatchNorm(bn_x)), bn_x laid
     *              out like y.  The epilogue recomputes xhat = (bn_x - bn_mean) * bn_invstd and the activation's sign from
     *              xhat * bn_gamma + bn_beta (the expression of the forward pass: the same bits), applies the activation's backward
     *              (y = t > 0 ? y : y * gate_slope, as `gate` would with the stored activation), and planes 0 / 1 become sum y |
     *              sum y * xhat (planes 2 .. 5 unused): the two sums of the BatchNorm backward (d beta, d gamma;
     *              vpho_bn_train_backward_stats_f32).  `gate` with bn_gamma / bn_beta: the stored activation is the fall-back of a
     *              kernel without the epilogue (ABI 13).  `gate` without bn_gamma / bn_beta: the sign comes from the stored activation
     *              as usual and only xhat is recomputed: the closing activation of a residual block, lrelu(BatchNorm(x) + shortcut),
     *              whose sign bn_x alone does not determine.
     * Served by the direct-to-LDS kernels' 16-byte epilogue: no splits / pixel list / groups / bf16 planes.  Where the kernel chosen for the
     * shape has no such epilogue (a forced tile, more M-tiles than stats_cap), a launch with `gate` uses the stored gate and reports
     * stats_rows = 0; with bn_x and no `gate` the call fails instead of dropping the gate. */
    float* stats;
    int* stats_rows;
    int stats_cap;
    const float* bn_x; const float* bn_mean; const float* bn_invstd; const float* bn_gamma; const float* bn_beta;
} vpho_conv_desc;
/* Limits: Cin, x_ld multiples of 4, 16-byte aligned x / w; x and w (all splits included) below 3.9 GB each (32-bit buffer offsets). */
VPHO_API int vpho_conv2d_nhwc_f32(const vpho_conv_desc* d, void* stream);
/* Winograd F(2x2, 3x3) form of a 3x3 / stride 1 / padding 1 convolution (+ bias, LeakyReLU): u = G g G^T, fp32, stage-tiled as
 * (Cin/8, 16 frequencies, Cout, 8 input channels) by model/pack.py::winograd_weights; 2.25 x fewer multiply-adds on the matrix cores, input / output transforms inside the kernel
 * (csrc/conv_winograd.hip).  Needs even H, W, Cin % 16 == 0, Cout % 64 == 0.  Results differ from vpho_conv2d_nhwc_f32 by fp32 rounding
 * of the transforms (~1e-6 relative). */
VPHO_API int vpho_conv3x3_winograd_nhwc_f32(const float* x, const float* u, const float* bias, int N, int H, int W, int Cin, int x_ld, int Cout,
                                   float out_slope, float* y, int y_ld, void* stream);
/* The same convolution on RoI windows only (the FPN smoothing convolutions, backbone_FPN_HFL.py:105-108, whose maps are read only
 * through RoIAlign, VPHO.py:126-129): wins = the (N,5) window table of vpho_roi_windows_i32, tile_base (N+1 ints, written by
 * vpho_winograd_window_tiles_i32) = first tile of every image on the list of 2 x 2 output tiles -- on each image's EVEN pixel grid,
 * so every pixel comes from the same 4 x 4 patch as in the full-map launch: bit-identical -- that touch its window.  y_rows is the
 * COMPACT (rows, Cout) matrix vpho_roi_align_window_nhwc_f32 reads; x is the ordinary (N,H,W,x_ld) map, of which only the windows
 * dilated by one pixel need to hold data.  Device-side lists: the grid is sized for all tiles, blocks past the last live tile exit
 * (no host round trip, replays in a HIP graph with new boxes).  tiles_hint (0 = unknown) only feeds the profiling counters. */
/* GROUPED form (ABI version 11): `groups` independent convolutions of the same shape in one launch (the twin hand / object branches):
 * group g reads x + g*x_group (floats; 0 = every group reads the same input), u + g*16*Cout*Cin, bias + g*Cout and writes images
 * [g*N, (g+1)*N) of y (groups*N, H, W, y_ld).  Bit-identical to `groups` single launches. */
VPHO_API int vpho_conv3x3_winograd_grouped_nhwc_f32(const float* x, long long x_group, const float* u, const float* bias, int groups, int N, int H, int W,
                                           int Cin, int x_ld, int Cout, float out_slope, float* y, int y_ld, void* stream);
VPHO_API int vpho_winograd_window_tiles_i32(const int* wins, int N, int* tile_base, void* stream);
/* ... and with the window pixels written IN PLACE into the ordinary (N,H,W,y_ld) map y, every other pixel of y left untouched (the
 * input gradient of an FPN smoothing convolution: non-zero only in the RoI windows dilated by the 3x3 halo; the caller zeroes y) */
VPHO_API int vpho_conv3x3_winograd_scatter_nhwc_f32(const float* x, const float* u, const float* bias, int N, int H, int W, int Cin, int x_ld, int Cout,
                                           float out_slope, const int* wins, const int* tile_base, float* y, int y_ld, void* stream);
/* Training (weights change every step): u on the DEVICE from the packed 3x3 weights (Cout, 9*Cin) -- for the forward convolution
 * (for_input_gradient = 0: u is (Cin/8, 16, Cout, 8)) or for its input-gradient convolution, the 3x3 convolution of dY with the
 * spatially flipped, channel-transposed weights (1: u is (Cout/8, 16, Cin, 8)); fp64 arithmetic, rounded once.  The gate variant
 * of the convolution fuses the backward of the LeakyReLU that produced the convolution's input (torch autograd of nn.LeakyReLU in
 * Bottleneck / Residual, backbone_FPN_HFL.py:326, encoding.py:21-36): y = gate > 0 ? y : gate_slope * y, gate laid out like y. */
VPHO_API int vpho_winograd_weights_f32(const float* w_packed, int Cout, int Cin, int for_input_gradient, float* u, void* stream);
/* the same for a list of weight tensors in one launch (ABI version 9).  segments: device array of n_segments records
 * { const float* w_packed; float* u; int32 Cout, Cin, for_input_gradient, first_block; } (32 bytes) with first_block = running sum of
 * ceil(Cout * Cin / 256) over the preceding records, total_blocks = that sum over all records; every record as for the single call
 * (the convolution's input channels a multiple of 16) -- not checked on the device. */
VPHO_API int vpho_winograd_weights_multi_f32(const void* segments, int n_segments, long long total_blocks, void* stream);
VPHO_API int vpho_conv3x3_winograd_gate_nhwc_f32(const float* x, const float* u, const float* gate, float gate_slope, int N, int H, int W, int Cin,
                                        int x_ld, int Cout, float* y, int y_ld, void* stream);
/* Full-map Winograd convolution with the BatchNorm reductions of vpho_conv_desc.stats in its epilogue (ABI version 13): stats =
 * [ceil(N*H*W/256)][6][Cout] floats, row t = the sums over the 256 output pixels of tile block t (64 tiles of 2 x 2); returns the number of
 * rows through *stats_rows (host).  bn_x == NULL: the forward convolution (bias, out_slope as above; sum v | sum v^2 | pivot |
 * sum (v - pivot) | sum (v - pivot)^2 | count of the stored values, the pivot a value of the block).
 * bn_x != NULL: the input-gradient convolution of the gate variant with the gate recomputed from bn_x (laid out like y, leading dimension
 * y_ld) and the BatchNorm vectors -- y = (xhat * gamma + beta > 0) ? y : gate_slope * y, sums y | y * xhat -- see vpho_conv_desc. */
VPHO_API int vpho_conv3x3_winograd_stats_nhwc_f32(const float* x, const float* u, const float* bias, int N, int H, int W, int Cin, int x_ld, int Cout,
                                         float out_slope, float* y, int y_ld, float* stats, int stats_cap, int* stats_rows, const float* bn_x,
                                         const float* bn_mean, const float* bn_invstd, const float* bn_gamma, const float* bn_beta,
                                         float gate_slope, void* stream);
VPHO_API int vpho_conv3x3_winograd_rows_nhwc_f32(const float* x, const float* u, const float* bias, int N, int H, int W, int Cin, int x_ld, int Cout,
                                        float out_slope, const int* wins, const int* tile_base, int tiles_hint, float* y_rows, int y_ld,
                                        void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Score network (GenPose-style conditional denoiser) and the probability-flow ODE sampler.
 * Replaces lib/model/denoiser.py:68-82 (BaseDenoiser.forward with ManoPoseHead2 :176-179 / ObjHead2 :244-247 and
 * parallel_linear.py:27-35) and lib/model/score_based_model.py:45-105 (cond_ode_sampler: scipy solve_ivp RK45,
 * rtol/atol controller, dense output on t_eval, final reverse-diffusion denoise step) with sde.py:15-28 (VE SDE).
 *
 * Weight layout (packed once by the caller from the reference state_dict):
 *   t_W[64]                     t_encoder.0.W
 *   t_w[128][128], t_b[128]     t_encoder.1.{weight,bias}            (row-major [out][in])
 *   pe0_w[256][Dp], pe0_b[256]  pose_encoder.0 (input dim D zero-padded to Dp, Dp % 4 == 0)
 *   pe2_w[256][256], pe2_b[256] pose_encoder.2
 *   w1_t[128][NH]               head.head.0.weight[n, 0:128,   j] at [k][n*256+j]         NH = nheads*256
 *   w1_p[NH][256]               head.head.0.weight[n, 128:384, j] at [n*256+j][k]
 *   w1_f[NH][1024], b1[NH]      head.head.0.weight[n, 384:1408, j] at [n*256+j][k]; head.head.0.bias
 *   w2[NH][4]                   head.head.2.weight[n, j, 0:3] padded to 4;  b2[nheads*3] head.head.2.bias
 * The 1408-wide first layer is evaluated as  feat-part (once per image, `cimg`) + t-part (once per evaluation)
 * + pose-part (per row, fp32 MFMA) -- algebraically the same sum (SURVEY.md 7 "algebraic opportunity").
 */
typedef struct {
    int D, Dp, nheads;
    const float *t_W, *t_w, *t_b, *pe0_w, *pe0_b, *pe2_w, *pe2_b, *w1_t, *w1_p, *w1_f, *b1, *w2, *b2;
    /* Optional, opt-in (NULL / 0 = the fp32-MFMA score head, the default and the path parity is stated on): w1_p as three bf16
     * planes [nheads][3][256][256] with w1_p = plane0 + plane1 + plane2 exactly (plane0 = bf16(w), plane1 = bf16(w - plane0), ...),
     * split_terms = 6 or 9 cross products per fp32 product on the bf16 matrix cores, fp32 accumulation (csrc/score_ode.hip). */
    const void* w1_p_split;
    int split_terms;
} vpho_score_weights;

/* bytes of scratch `vpho_score_eval` / `vpho_ode_sample` need for R = bs*S rows */
VPHO_API long long vpho_score_workspace_bytes(const vpho_score_weights* w, int bs, int S);

/* One score evaluation s(x, t | feat) for R = bs*S rows (row r belongs to image r / S).
 * feat_img: [bs][1024], x: [R][D] fp32, t: scalar shared by all rows, out: [R][D] fp32.  (denoiser.py:68-82) */
VPHO_API int vpho_score_eval(const vpho_score_weights* w, const float* feat_img, int bs, int S, const float* x, float t,
                    float* out, void* workspace, long long workspace_bytes, void* stream);

typedef struct {
    int nfev;            /* score-network evaluations incl. the final denoise call */
    int n_accepted, n_rejected;
    int nan_count;       /* NaN score entries replaced by 0 (score_based_model.py:69-71) */
    int status;          /* 0 ok, 1 step size underflow */
    int n_log;           /* entries written to step_log_host: (t, h, error_norm, accepted) per attempted step */
} vpho_ode_stats;

/* Full cond_ode_sampler run.  init_x: [R][D] fp32 prior draw (already scaled by sigma(T0)).
 * xs_out: [R][num_steps][D] dense output at t_eval = linspace(T0, eps, num_steps), fp64 if xs_is_f64 else fp32
 * (the reference casts the hand trajectory to fp32 right after sampling, VPHO.py:243); x_out: [R][D] final sample
 * after the denoise step, fp64 if x_is_f64 else rounded to fp32 the same way.  scipy's scalar step controller
 * (select_initial_step, accept/reject, step-size factor, t_eval stamps) runs in one-thread kernels on a control block in the
 * workspace; the call enqueues the expected number of attempts plus the denoise step and waits for `stream` ONCE (more
 * attempts are added two at a time if the solve is not finished).  With the environment variable VPHO_RK_HOST=1 (or
 * num_steps > 1024) the controller runs on the host instead and the call synchronises once per attempted step.
 * stats_host / step_log_host are host memory (step_log_host may be NULL; capacity in entries of 4 doubles). */
VPHO_API int vpho_ode_sample(const vpho_score_weights* w, const float* feat_img, int bs, int S, const float* init_x,
                    double T0, double eps, int num_steps, double rtol, double atol,
                    void* xs_out, int xs_is_f64, void* x_out, int x_is_f64,
                    void* workspace, long long workspace_bytes,
                    vpho_ode_stats* stats_host, double* step_log_host, int step_log_cap, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HBM-bound glue of the feature path (NHWC fp32).  c_off / ld* let a kernel write straight into a channel slice of a
 * wider (concatenation) buffer.
 */
/* rgb (N,C,H,W) -> (N,H,W,ldy) with channels >= C zero-filled (input of the 7x7 stem, backbone_FPN_HFL.py:206) */
VPHO_API int vpho_nchw_to_nhwc_f32(const float* x, int N, int C, int H, int W, float* y, int ldy, void* stream);
/* (N,H,W,C | ldx) -> (N,C,H,W): heat-map outputs (VPHO.py:232-233) and Encoder's x.flatten(1) (encoding.py:72) */
VPHO_API int vpho_nhwc_to_nchw_f32(const float* x, int N, int H, int W, int C, int ldx, float* y, void* stream);
/* nn.MaxPool2d (backbone_FPN_HFL.py:209 k3 s2 p1; encoding.py:54 k2 s2) */
VPHO_API int vpho_maxpool_nhwc_f32(const float* x, int N, int H, int W, int C, int k, int stride, int pad, float* y, void* stream);
/* F.interpolate(mode='bilinear', align_corners=False); accumulate=1 gives FPN._upsample_add (backbone_FPN_HFL.py:66-68),
 * accumulate=0 with c_off the heat-map 64->32 resize into the encoder input (VPHO.py:143-144,148-149) */
VPHO_API int vpho_resize_bilinear_nhwc_f32(const float* x, int N, int H, int W, int C, int ldx, int OH, int OW,
                                  float* y, int ldy, int c_off, int accumulate, void* stream);
/* torchvision.ops.roi_align(aligned=False, sampling_ratio=-1), one box per image, boxes (N,4) xyxy (VPHO.py:125-128);
 * flip_w[n] != 0 mirrors the output along W (flip_tensor_by_mask_index, VPHO.py:138) */
VPHO_API int vpho_roi_align_nhwc_f32(const float* feat, int N, int H, int W, int C, const float* boxes, float spatial_scale,
                            int out_size, const unsigned char* flip_w, float* out, int ldo, int c_off, void* stream);
/* Demand-driven FPN output.  The stride-4 maps of FPN.forward (backbone_FPN_HFL.py:105-109) are read ONLY by the RoIAligns of
 * VPHO.py:126-129, so each branch's last convolution is computed on the pixels its image's boxes can sample and nowhere else --
 * the same values, about half the pixels at the README config's box sizes (dexycb6.py:346-356: boxes = 1.15 / 1.10 x the tight
 * key-point boxes).  vpho_roi_windows_i32: per image the window = union over boxes_a[n], boxes_b[n] (NULL = one box) of the rows /
 * columns a bilinear sample of torchvision's roi_align can weigh; wins (N,5) = (first compact row, y0, x0, w, h), row_map = linear
 * pixel index (n*H + y)*W + x of every window pixel in compact order, *row_count their number; dilate > 0 widens every window by
 * that many pixels (the 3x3 halo: the lateral 1x1 convolution and the top-down add that feed the last convolution run on the
 * windows dilated by 1, stored in place -- vpho_conv_desc.rows_scatter).  All device-side: feed row_map /
 * row_count to vpho_conv_desc and wins to vpho_roi_align_window_nhwc_f32, which reads the compact (rows, C) matrix with the
 * arithmetic of vpho_roi_align_nhwc_f32 (bit-identical outputs, tests/test_gpu_glue.py). */
VPHO_API int vpho_roi_windows_i32(const float* boxes_a, const float* boxes_b, int N, int H, int W, float spatial_scale, int dilate,
                         int* wins, int* row_map, int* row_count, void* stream);
/* vpho_resize_bilinear_nhwc_f32 on the listed output pixels only (FPN._upsample_add inside the dilated windows) */
VPHO_API int vpho_resize_bilinear_rows_nhwc_f32(const float* x, int N, int H, int W, int C, int ldx, int OH, int OW, float* y, int ldy, int c_off,
                                       int accumulate, const int* row_map, const int* row_count, int rows_hint, void* stream);
VPHO_API int vpho_roi_align_window_nhwc_f32(const float* feat_rows, const int* wins, int N, int H, int W, int C, const float* boxes,
                                   float spatial_scale, int out_size, const unsigned char* flip_w, float* out, int ldo, int c_off, int rows_hint,
                                   void* stream);
/* the same pooling pass with TWO destinations (each with its own optional W-flip flags): the object branch pools bbox_obj_rect twice,
 * plain for the heat-map head and flipped for left hands into the encoder input (VPHO.py:126-138) -- one read of the map, values
 * bit-identical to two vpho_roi_align_window_nhwc_f32 calls */
VPHO_API int vpho_roi_align_window_dual_nhwc_f32(const float* feat_rows, const int* wins, int N, int H, int W, int C, const float* boxes,
                                        float spatial_scale, int out_size, const unsigned char* flip_w, float* out, int ldo, int c_off,
                                        const unsigned char* flip_w2, float* out2, int ldo2, int c_off2, int rows_hint, void* stream);
/* align_hm_to_bbox_rectangle (VPHO.py:333-346, transposing, quirk Q2) (+ optional W flip, VPHO.py:139) */
VPHO_API int vpho_align_heatmap_nhwc_f32(const float* hm, int N, int size, int C, const float* bbox, const float* bbox_rect,
                                const unsigned char* flip_w, float* out, void* stream);
/* NeRF embedding of gravity (cross_module.py:8-46), x negated where flip_x (VPHO.py:167); out (N,64), column 63 = 0 */
/* y = act(x . w^T + bias) of a SMALL linear layer with the products and the sum in double, rounded to fp32 once (ABI version 11): the
 * regression head head_mano.py:61-70, whose output is normalised into half of the cascade's candidates (aggregation.py:120-126) -- see
 * csrc/misc.hip.  x (rows, ld_x >= cin), w (cout, cin) packed, y (rows, ld_y >= cout); cin <= 4096. */
VPHO_API int vpho_linear_acc64_f32(const float* x, int rows, int cin, int ld_x, const float* w, const float* bias, int cout, float out_slope,
                          float* y, int ld_y, void* stream);
VPHO_API int vpho_nerf_embed_f32(const float* g, int N, const unsigned char* flip_x, float* out, void* stream);
/* (bs,65,512) token tensor of CrossModule.forward (cross_module.py:124-133) incl. the positional code of the BATCH index */
VPHO_API int vpho_cross_tokens_f32(const float* proj_hand, const float* proj_obj, const float* grav_emb, const float* pe,
                          int bs, float* out, void* stream);
/* multi-head attention core over the first axis of qkv (S,B,3E) (nn.MultiheadAttention inside cross_module.py:104-107) */
VPHO_API int vpho_mha_f32(const float* qkv, int S, int B, int E, int nhead, float* out, void* stream);
/* the same with nn.MultiheadAttention's dropout on the attention probabilities (training): drop_mask [B*nhead][S][S] = keep / (1 - p),
 * applied after the soft-max and before P V; NULL = no dropout */
VPHO_API int vpho_mha_dropout_f32(const float* qkv, int S, int B, int E, int nhead, const float* drop_mask, float* out, void* stream);
/* out = LayerNorm(x + r) (post-norm TransformerEncoderLayer) */
VPHO_API int vpho_add_layernorm_f32(const float* x, const float* r, const float* gamma, const float* beta, long long rows, int E,
                           float eps, float* out, void* stream);
/* HeadPhysics: |scale| * normalise(softmax(softmax(logits)) . friction-cone anchors) (physics.py:546-557,700-712).
 * Output row r reads token row (r / group) * group_stride + r % group (+ off_scale | off_logits) of the MLP outputs, so the
 * 32 hand / 32 object tokens are picked out of the (bs, 65, .) transformer output without a copy. */
VPHO_API int vpho_force_local_f32(const float* scale, int ld_scale, const float* logits, int ld_logits, const float* anchor,
                         float friction, long long rows, int group, int group_stride, int off_scale, int off_logits,
                         float* out, void* stream);
/* matrix_to_axis_angle(rotation_6d_to_matrix(x)) for rows of rot_per_row rotations (head_mano.py:66-69, VPHO.py:314-324) */
VPHO_API int vpho_rot6d_to_axis_angle_f32(const float* x, long long rows, int rot_per_row, int ldx, float* out, int ldo, void* stream);
/* out[row, 48:58] = betas[row / rows_per_image] (VPHO.py:318-319,325-326) */
VPHO_API int vpho_append_betas_f32(const float* betas, long long rows, long long rows_per_image, float* out, int ldo, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * MANO forward kinematics (manopth.ManoLayer as configured at head_mano.py:48-55; metres, head_mano.py:78-87).
 * posedirs_t is the pose-blend table transposed to [135][778*3] (coalesced over vertices).
 */
typedef struct {
    const float *v_template;   /* [778][3]      */
    const float *shapedirs;    /* [778][3][10]  */
    const float *posedirs_t;   /* [135][778*3]  */
    const float *J_regressor;  /* [16][778]     */
    const float *weights;      /* [778][16]     */
    /* ABI version 6, optional (NULL: read the columns from posedirs_t): the 30 pose-blend columns of the 10 finger-tip vertices
     * (5 manopth tips 745, 317, 444, 556, 673, then 5 HO3D tips 728, 353, 442, 576, 694; column = tip * 3 + c) gathered into one
     * contiguous [135][30] table -- the joints-only launches of the heat-map cascade read nothing else of the 1.26 MB table */
    const float *tip_posedirs_t;
    /* ABI version 7, optional (NULL: big launches with vertices take the packed-FMA kernel): the pose-blend table in the operand order
     * of the fp32 matrix-core kernel, zero padded to 136 rows and 800 vertices: [25 vertex tiles][17 groups of 4 k steps][3][2][32][4],
     * element (t, g, j, lh, li, e) = posedirs_t[k][(32 t + li) * 3 + c] with f = 4 j + e, k = 2 (4 g + f / 3) + lh, c = f % 3 --
     * a lane's B fragments of four k steps are three aligned 16-byte loads, consecutive lanes read consecutive 16 bytes */
    const float *posedirs_mfma;
} vpho_mano_tables;
/* per image: v_shaped (n_img,778,3), J (n_img,16,3) from betas (n_img,10) */
VPHO_API int vpho_mano_shape_f32(const vpho_mano_tables* t, const float* betas, int n_img, float* v_shaped, float* J, void* stream);
/* per hand: pose rows of ld_pose floats (first 48 = axis-angle); hand h uses image h / hands_per_image.
 * verts may be NULL (joints only).  ho3d_per_image (optional) selects hand_fn.get_joint_aligned_with_HO3D ordering. */
VPHO_API int vpho_mano_fk_f32(const vpho_mano_tables* t, const float* pose, int ld_pose, long long n_hands, int hands_per_image,
                     const float* v_shaped, const float* J, const unsigned char* ho3d_per_image,
                     float* verts, float* joints, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Aggregation (lib/model/aggregation.py HOI_Aggregator.__call__ :1167-1353 and callees; lib/utils/transform_fn.py:101-125;
 * lib/utils/physics_fn.py:224-257).  Top-k order: value descending, ties by ascending candidate index.
 */
typedef struct { const float* kpt; const float* vert; const float* com; int n_kpt, n_vert, n_obj; } vpho_obj_tables;
    /* kpt [n_obj][n_kpt][3], vert [n_obj][n_vert][3], com [n_obj][3]   (head_object.py:13-33) */
typedef struct { const int* face_idx; const float* anchor_weight; const float* vert2joint; const int* skeleton; } vpho_anchor_tables;
    /* face_idx [32][3], anchor_weight [32][2], vert2joint [21][778], skeleton [32][2]   (physics_fn.py:120-171) */

/* pose (bs,2S,48): [S diffusion | S regression with the diffusion wrist] (aggregation.py:120-126,140-143) */
VPHO_API int vpho_hand_candidates_f32(const float* diff_pose, int ld_diff, const float* reg_pose, int bs, int S, float* pose, void* stream);
/* hv (bs,C,n_obs): bicubic heat-map value of each observed joint of each candidate (aggregation.py:196-213);
 * joints (bs,C,21,3) root-relative, heatmap (bs,J,H,W) planar; observe_host is a HOST int array */
VPHO_API int vpho_hand_heat_f32(const float* joints, const float* root, const float* Kmat, const float* bbox, const float* heatmap,
                       int bs, int C, int J, int H, int W, const int* observe_host, int n_obs, float* out, void* stream);
/* one cascade level (aggregation.py:215-269): score -> top-k -> weighted quaternion mean -> broadcast into all candidates.
 * val/idx: [bs][F][k] with F = 1 (level 0) or 5, in torch.topk's order (larger score first; equal scores: smaller index first);
 * topk_pose (optional) [bs][k][F][3]; score_out (optional) [bs][C][F] = the level score of EVERY candidate exactly as ranked
 * (aggregation.py:215-218,244-247: sum over the observed joints at level 0, per-finger mean at levels 1-3) */
VPHO_API int vpho_hand_fuse_level_f32(const float* hv, int n_obs, float* pose, int bs, int C, int k, int level,
                             float* val, int* idx, float* topk_pose, float* score_out, void* stream);
/* generic wavefront top-k: element c of row (o,f) at scores[(o*n + c)*F + f]; val/idx [o][f][k] */
VPHO_API int vpho_topk_f32(const float* scores, int rows_outer, int n, int F, int k, float* val, int* idx, void* stream);
VPHO_API int vpho_topk_weights_f32(const float* val, int rows, int k, float* w, void* stream);
/* select_topk_object_by_heatmap score (aggregation.py:742-776); pose (bs,n,9) fp64.  vpho_obj_heat_score, vpho_obj_physics_score and
 * vpho_obj_verts_f32: an obj_id outside [0, n_obj) gives NaN for that image's outputs (no table row is read), as vpho_obj_pt2d_score */
VPHO_API int vpho_obj_heat_score(const double* pose, int n, const double* transl_override, const float* root, const vpho_obj_tables* t,
                        const int* obj_id, const unsigned char* is_right, const float* Kmat, const float* bbox,
                        const float* heatmap, int bs, int H, int W, float* score, void* stream);
VPHO_API int vpho_obj_cross_candidates(const double* pose, int n, const int* transl_idx, const int* rot_idx, int bs, int ko, double* cand, void* stream);
/* select_topk_object_by_physics3 score (aggregation.py:947-985) */
VPHO_API int vpho_obj_physics_score(const double* cand, int n, const float* root, const vpho_obj_tables* t, const int* obj_id,
                           const unsigned char* is_right, const float* force_point, const float* force_global, int bs,
                           float* score, void* stream);
/* fuse_topk + average_rot6d in fp64 (aggregation.py:729-740,50-56); source b (if given) is used where pick_b[b] != 0 */
VPHO_API int vpho_obj_fuse_f64(const double* pose, int n, const int* idx_a, const float* w_a, const int* idx_b, const float* w_b,
                      const unsigned char* pick_b, int bs, int k, double* fused, void* stream);
VPHO_API int vpho_obj_verts_f32(const double* pose, const float* root, const vpho_obj_tables* t, const int* obj_id,
                       const unsigned char* is_right, int bs, float* out, void* stream);
/* ForceAnchor.__call__ on (verts + root) and from_local_to_global (physics_fn.py:224-257, physics.py:362-371) */
VPHO_API int vpho_force_anchor_f32(const vpho_anchor_tables* t, const float* verts, const float* root, const float* force_local,
                          long long n_hands, int hands_per_image, float* force_point, float* force_global, void* stream);
/* aggregation.py:1306-1325 / :561-596 / :598-617 */
VPHO_API int vpho_hand_phys_candidates_f32(const float* agg_pose, int ld_agg, const float* betas, const float* topk_pose, int bs, int k,
                                  float* out, void* stream);
VPHO_API int vpho_hand_phys_score_f32(const float* force_point, const float* force_global, const float* obj_vert, int n_vert,
                             int bs, int n_cand, float* finger_score, void* stream);
VPHO_API int vpho_hand_phys_fuse_f32(const float* cand, int n_cand, const int* idx, int bs, int k, float* out, void* stream);

/* The ablation aggregators (--aggregation_mode_hand / --aggregation_mode_obj other than heatmap_cascade), appended
 * within ABI version 13.  The object side fuses with vpho_obj_fuse_f64 (NULL weights).
 * vpho_heatmap_peak_f32 (aggregation.py:313-323, :1025-1035): per map of heatmap [n_maps][H][W] the arg-max in torch.argmax's order
 * (first maximum; a NaN is a maximum), as the pair the reference reads from its transposed grid: peak [n_maps][2] =
 * (X[ind / W], X[ind % W]), X[i] = i / (W - 1) * 2 - 1; ind [n_maps] (optional) the flat index.  H == W is required. */
VPHO_API int vpho_heatmap_peak_f32(const float* heatmap, long long n_maps, int H, int W, float* peak, int* ind, void* stream);
/* select_by_2D_pt score of the hand (aggregation.py:303-327): joints [bs][C][21][3] root-relative (vpho_mano_fk_f32), peak [bs][21][2];
 * score [bs][C][21] = -distance of each projected joint to its map's peak in the bbox's (-1, 1) frame (per_joint != 0, the layout
 * vpho_topk_f32 takes with F = 21) or its sum over the joints [bs][C]; fp32 */
VPHO_API int vpho_hand_pt2d_score_f32(const float* joints, const float* root, const float* Kmat, const float* bbox, const float* peak,
                             int bs, int C, int per_joint, float* score, void* stream);
/* the same for the object's key-points (aggregation.py:1015-1039): pose [bs][n][9] fp64, peak [bs][t->n_kpt][2]; score [bs][n], the
 * chain in fp64 like vpho_obj_heat_score; an obj_id outside [0, n_obj) gives NaN scores */
VPHO_API int vpho_obj_pt2d_score(const double* pose, int n, const float* root, const vpho_obj_tables* t, const int* obj_id,
                        const unsigned char* is_right, const float* Kmat, const float* bbox, const float* peak, int bs,
                        float* score, void* stream);
/* quaternion mean of WHOLE hand poses (aggregation.py:221-233 with all 48 parameters, :331-336, :401-405): pose rows of ld_pose
 * floats (first 48 = axis-angle), C per image; idx [bs][n] (NULL: candidates 0 .. n-1), w [bs][n] (NULL: unweighted);
 * fused [bs][48].  n <= 2 C.  An index outside [0, C) is not read: that image's row is NaN. */
VPHO_API int vpho_hand_pose_fuse_f32(const float* pose, int ld_pose, int C, const int* idx, const float* w, int bs, int n, float* fused,
                            void* stream);
/* 2D_pt_joint (aggregation.py:357-362): fused [bs][21][3] = mean over idx [bs][21][k] (vpho_topk_f32, F = 21) of joints [bs][C][21][3] */
VPHO_API int vpho_hand_joint_gather_mean_f32(const float* joints, const int* idx, int bs, int C, int k, float* fused, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Evaluation metrics on the device: TesterHand.criterion_MJE_PAMJE (lib/engine/test.py:657-680) with
 * rigid_align_AtoB (lib/utils/transform_fn.py:43-66).  pd, gt: [n_img][n_pts][3] fp32 (metres); outputs per image the
 * mean point error, the mean error after similarity (Procrustes) alignment of pd onto gt, optionally every point's error. */
VPHO_API int vpho_hand_metrics_f32(const float* pd, const float* gt, int n_img, int n_pts, float* mean_err, float* pa_mean_err,
                          float* per_point, void* stream);

/* Object evaluation metrics on the device: TesterObject.__call__ (lib/engine/test.py:240-352) for a single
 * hypothesis per image -- criterion_MCE_OCE (:354-374), criterion_MCE2 / compute_obj_metrics_dexycb (:398-414,155-193),
 * criterion_ADD_REP (:425-458), cal_ADD01d / cal_REP5 (:505-519), criterion_FSCORE (:460-503).
 * Tables are the fp64 YCB_MESHES entries (lib/dataset/base.py:222-244); pd_rt / gt_rt [n_img][3][4] and cam_intr [n_img][3][3]
 * fp64 (obj_9D_to_mat + root joint, train_diff_hand_obj.py:594-597); obj_id [n_img] indexes the tables; max_verts >= the
 * largest per-object vertex count.  out [n_img][16] = MCE, OCE, MCE2, ADD, ADD-S, ADD<0.1d, ADD-S<0.1d, REP, REP<5px,
 * Chamfer-L2, F-score @ 2 mm, 5 mm, 10 mm, 2 cm, 5 cm, 10 cm (metres / pixels / {0,1} / [0,1]). */
typedef struct vpho_obj_metric_tables {
    const double* bbox3d;          /* [n_obj][8][3] */
    const double* verts_sampled;   /* [n_obj][n_sampled][3] */
    const double* verts;           /* [vert_offset[n_obj]][3], objects concatenated */
    const int* vert_offset;        /* [n_obj + 1] */
    const double* diameter;        /* [n_obj] */
    int n_obj, n_sampled;
} vpho_obj_metric_tables;
/* obj_9D_to_mat (lib/utils/transform_fn.py:85-90) with the root joint added to the translation (Trainer.postprocess,
 * train_diff_hand_obj.py:578-597): pose9 [n][9] fp64 = [rot6d | t], root_joint [n][3] fp32 -> rt [n][3][4] fp64. */
VPHO_API int vpho_obj_9d_to_rt_f64(const double* pose9, const float* root_joint, int n, double* rt, void* stream);
VPHO_API long long vpho_obj_metrics_workspace_bytes(const vpho_obj_metric_tables* t, int n_img, int max_verts);
VPHO_API int vpho_obj_metrics_f64(const vpho_obj_metric_tables* t, const double* pd_rt, const double* gt_rt, const double* cam_intr,
                         const int* obj_id, int n_img, int max_verts, double* out, void* workspace, long long workspace_bytes,
                         void* stream);

/* Multi-hypothesis evaluation: every one of the n_hyp sampled candidates of an image scored against the image's ground truth,
 * which is broadcast over the candidates (test_diff_hand / test_diff_object with is_eval_best, train_diff_hand_obj.py:454-523).
 * vpho_hand_metrics_multi_f32: TesterHand.__call__ on pd_* [n_img][n_hyp][P][3] (lib/engine/test.py:589-597,657-679).
 *   pd [n_img][n_hyp][n_pts][3] fp32 in the model frame, as predict returns diff_final_hand_joint / diff_final_hand_vert; the
 *   postprocess of train_diff_hand_obj.py:578-602 (x un-flipped where !is_right, root_joint [n_img][3] added) is applied on load.
 *   gt [n_img][n_pts][3]; is_right [n_img] (0 / 1).  mean_err, pa_mean_err [n_img][n_hyp]: MJE and PA-MJE in metres.
 * vpho_obj_metrics_multi_f64: TesterObject.__call__ (test.py:240-503) once per candidate slice pd_rt[:, s], and
 *   TesterObject.postprocess (test.py:522-567).  pd_rt [n_img][n_hyp][3][4] fp64; gt_rt, cam_intr, obj_id, max_verts as in
 *   vpho_obj_metrics_f64.  out [n_img][n_hyp][16] in the column order of vpho_obj_metrics_f64; best [n_img][16] = per-image
 *   min over the candidates (max for ADD<0.1d, ADD-S<0.1d, REP<5px and the F-scores, test.py:529-538); mean [n_img][16] =
 *   mean over the candidates.  best and mean may be NULL.  The workspace is O(n_img * n_hyp); its size comes from
 *   vpho_obj_metrics_multi_workspace_bytes (-1 on a bad argument).  Deterministic: fixed reduction orders throughout. */
VPHO_API int vpho_hand_metrics_multi_f32(const float* pd, const float* gt, const float* root_joint, const unsigned char* is_right, int n_img,
                                int n_hyp, int n_pts, float* mean_err, float* pa_mean_err, void* stream);
VPHO_API long long vpho_obj_metrics_multi_workspace_bytes(const vpho_obj_metric_tables* t, int n_img, int n_hyp, int max_verts);
VPHO_API int vpho_obj_metrics_multi_f64(const vpho_obj_metric_tables* t, const double* pd_rt, const double* gt_rt, const double* cam_intr,
                               const int* obj_id, int n_img, int n_hyp, int max_verts, double* out, double* best, double* mean,
                               void* workspace, long long workspace_bytes, void* stream);

/* Hand benchmark metrics for every sampled hypothesis (--eval_hand_bench), appended within ABI version 13.  They
 * replace nothing in the reference: the definitions are those of the FreiHAND / HO3D leaderboards' eval.py (F-score at two distances,
 * AUC of the PCK curve), the alignment is rigid_align_AtoB (lib/utils/transform_fn.py:43-66) as in vpho_hand_metrics_multi_f32.
 * vpho_hand_bench_multi_f32: pd, gt, root_joint, is_right as in vpho_hand_metrics_multi_f32 (postprocess applied on load); A = the
 *   postprocessed hypothesis, B = the ground truth, A^ = the aligned A (fp64).  Per-point errors e = |X - B| in fp64 for X = A, A^.
 *   auc_thresh [n_thresh] ascending fp64 thresholds (metres), auc_g [n_thresh + 1]: auc_g[c] = the normalised trapezoid integral of the
 *   step 1[e <= t] for a point with c = #{j : e <= auc_thresh[j]}; AUC = (sum_p auc_g[c_p]) / n_pts.  With with_fscore != 0 also, for
 *   th in (f_thresh_lo, f_thresh_hi): precision = #{d1 < th} / n_pts, recall = #{d2 < th} / n_pts (d1: B's points to their nearest point of
 *   X, d2: X's points to their nearest point of B; fp32 brute force on points centred on B's centroid), F = 2 p r / (p + r), 0 when
 *   p + r = 0.  values [n_img][n_hyp][6] = AUC, PA AUC, F@lo, F@hi, PA F@lo, PA F@hi (the four F entries NaN when with_fscore == 0).
 *   counts (may be NULL) [n_img][n_hyp][10] int32 = #{d1 < lo}, #{d1 < hi}, #{d2 < lo}, #{d2 < hi} raw, the same four aligned (0 when
 *   with_fscore == 0), sum_p c_p raw, sum_p c_p aligned.  A pair with a non-finite coordinate gives NaN values (counts 0).
 *   3 <= n_pts <= 1024, 2 <= n_thresh <= 256, n_img * n_hyp <= 2^31 - 1: anything else is an error before any launch.
 * vpho_hand_bench_table_f64: per [n_img][n_hyp][8] -> one [n_img][8] (hypothesis 0), best [n_img][8] (per-value MAXIMUM over the
 *   hypotheses), mean [n_img][8] (fp64 sum in ascending hypothesis order / n_hyp); a NaN hypothesis makes best and mean NaN.
 * Deterministic: fixed reduction orders, integer counts, no atomics. */
VPHO_API int vpho_hand_bench_multi_f32(const float* pd, const float* gt, const float* root_joint, const unsigned char* is_right, int n_img,
                              int n_hyp, int n_pts, double f_thresh_lo, double f_thresh_hi, const double* auc_thresh, const double* auc_g,
                              int n_thresh, int with_fscore, double* values, int* counts, void* stream);
VPHO_API int vpho_hand_bench_table_f64(const double* per, int n_img, int n_hyp, double* one, double* best, double* mean, void* stream);

/* Symmetry-aware object errors for every sampled hypothesis (--eval_symmetric), appended within ABI version 13.
 * vpho_obj_symmetry_multi_f64 replaces TesterObject.criterion_SMCE (lib/engine/test.py:377-398; its call at :258 is commented out as
 *   "very slow") over the padded symmetry table of TesterObject.__init__ (:204-226; get_symmetry_transformations :103-150,
 *   rotation_matrix :59-100 -- vpho_amd/symmetry.py builds it on the host), and adds the BOP toolkit's MSSD over the same table and the
 *   sampled vertices of criterion_ADD_REP (:425-458).  With S_k = (sym_R[k] | sym_t[k]), P = pd_rt[b][s], G = gt_rt[b] and
 *   D_k = P - G S_k (one 3x4 affine map per (hypothesis, k)):
 *     SMCE = min_k mean_c |D_k c| over the 8 corners bbox3d;  MSSD = min_k max_v |D_k v| over verts_sampled (any n_sampled >= 1).
 *   Every one of the K rows of the object's table takes part, the identity pads included (the reference indexes all of them too).
 *   per [n_img][n_hyp][3] = SMCE (m), MSSD (m), MSSD < 0.1 * diameter (0 / 1).  prune != 0 lets a lane abandon a symmetry once its
 *   running maximum reaches the smallest completed maximum of an earlier round of 256 symmetries; prune == 0 runs every pair in full;
 *   both return the same bits.  A hypothesis or ground truth with a non-finite entry, or an obj_id outside [0, n_obj), gives NaN, NaN, 0.
 *   1 <= K <= 4096, n_img * n_hyp <= 2^31 - 1: anything else is an error before any launch.
 * vpho_obj_symmetry_table_f64 (TesterObject.postprocess, test.py:522-567): per [n_img][n_hyp][3] -> one [n_img][3] (hypothesis 0), best
 *   [n_img][3] (min of SMCE and MSSD, max of the hit), mean [n_img][3] (fp64 sum in ascending hypothesis order / n_hyp).  NaN rows as in
 *   vpho_obj_metrics_multi_f64: best starts from hypothesis 0 and takes a later value only where `v < best` (`v > best` for the hit)
 *   holds, so a NaN hypothesis 0 gives NaN and a later NaN hypothesis is passed over; mean is NaN as soon as one hypothesis is (the
 *   hit of such a hypothesis is 0 and counts as a miss).
 * Deterministic: fixed reduction orders, no atomics, nothing depends on the order of the workgroups. */
typedef struct vpho_obj_symmetry_tables {
    const double* sym_R;           /* [n_obj][K][3][3] */
    const double* sym_t;           /* [n_obj][K][3], metres */
    const double* bbox3d;          /* [n_obj][8][3] */
    const double* verts_sampled;   /* [n_obj][n_sampled][3] */
    const double* diameter;        /* [n_obj] */
    int K, n_obj, n_sampled;
} vpho_obj_symmetry_tables;
VPHO_API int vpho_obj_symmetry_multi_f64(const vpho_obj_symmetry_tables* t, const double* pd_rt, const double* gt_rt, const int* obj_id,
                                int n_img, int n_hyp, int prune, double* per, void* stream);
VPHO_API int vpho_obj_symmetry_table_f64(const double* per, int n_img, int n_hyp, double* one, double* best, double* mean, void* stream);

/* Prediction records of --mode infer (Trainer.infer, lib/engine/train_diff_hand_obj.py:359-444): ONE launch turns the predict outputs of a
 * batch into fixed-layout per-image records, and ONE hipMemcpyAsync ships them to the host.  Replaces, per batch, the postprocess of
 * the four hand arrays (__postprocess_hand_vert, :598-602: x negated where !is_right, then + root_joint; one sign flip and one fp32 add
 * per element), `.astype(np.float16)` of the aggregated vertices (:383; round to nearest even, overflow to inf, subnormals kept),
 * __postprocess_obj_rt of agg_obj_6d (:593-596; the arithmetic of vpho_obj_9d_to_rt_f64, bit for bit) and to_numpy (:375-376).
 * Record of one image, vpho_infer_record_bytes(n_joint, n_vert) bytes (a multiple of 8; -1 on a bad argument):
 *   block A  fp32  reg_joint [n_joint][3] | reg_vert [n_vert][3] | agg_joint [n_joint][3] | agg_vert [n_vert][3]   camera frame
 *   block B  fp16  agg_vert of block A [n_vert][3], then zero padding to a multiple of 8 bytes
 *   block C  fp64  pd_obj_rt [3][4] = [R | t + root]
 * reg_* / agg_* [n_img][n_pts][3] fp32 in the model frame as predict returns them, agg_obj_6d [n_img][9] fp64, root_joint [n_img][3]
 * fp32, is_right [n_img] (0 / 1); n_vert must be even (block B is written two halves per dword).  records: device, n_img records.
 * records_host: pinned host memory or NULL; when given, the records are copied to it on `stream` behind the kernel (the caller
 * waits for the stream or an event on it before reading).  Deterministic; no workspace. */
VPHO_API long long vpho_infer_record_bytes(int n_joint, int n_vert);
VPHO_API int vpho_infer_pack_f32(const float* reg_hand_joint, const float* reg_hand_vert, const float* agg_hand_joint, const float* agg_hand_vert,
                        const double* agg_obj_6d, const float* root_joint, const unsigned char* is_right, int n_img, int n_joint,
                        int n_vert, void* records, void* records_host, void* stream);

/* Hand-object penetration and contact (--eval_physics).  The object meshes as per-triangle records
 * tri [tri_offset[n_obj]][VPHO_PEN_TRI_STRIDE] fp64, objects concatenated (vpho_amd/physics_eval.py builds them on the host):
 *   fields 0-18 in the object's hash frame (q = scale * p + translate, the mesh bbox mapped onto [0.5, 511.5]^3; corners t1, t2, t3):
 *     0-1 t3.xy, 2-5 A = (t1.x - t3.x, t2.x - t3.x; t1.y - t3.y, t2.y - t3.y) row-major, 6 sign(det A), 7 |det A|,
 *     8-9 t1.xy, 10-11 n.xy, 12 sign(n.z), 13 |n.z| with n = (t3 - t1) x (t2 - t1), 14 t1.z |n.z| (NaN where n.z == 0),
 *     15-18 the xy hash cells of the triangle's bbox (int-truncated, clamped to [0, 511]): x0, x1, y0, y1;
 *   fields 19-27 in the model frame (metres): corner a, b - a, c - a.
 * scale, translate [n_obj][3].
 * vpho_hand_obj_penetration_f64: verts [n][V][3] fp32 in the camera frame, obj_rt [n][3][4] fp64 [R | t] (model -> camera),
 * obj_id [n].  Per vertex p = R^T (v - t); inside(p) by the z-ray parity rule at resolution VPHO_PEN_RESOLUTION, d(p) = exact
 * distance to the nearest triangle; sd [n][V] = -d if inside else d (metres), inside [n][V] = 0 / 1; per_image [n][4] =
 * penetration depth (max d over the inside vertices, 0 if none), inside-vertex count, min sd, contact (min sd <= contact_thresh).
 * sd and inside may be NULL (then a stream-ordered temporary holds them).  An obj_id outside [0, n_obj) cannot be refused without a
 * host sync: its image gets NaN in sd and per_image and inside = 0 (vpho_amd.ops.HandObjectPenetration refuses such ids on the host).
 * n == 0 is a no-op.  Deterministic (max / min / count). */
#define VPHO_PEN_TRI_STRIDE 28
#define VPHO_PEN_RESOLUTION 512
typedef struct vpho_obj_mesh_tables {
    const double* tri;             /* [tri_offset[n_obj]][VPHO_PEN_TRI_STRIDE] */
    const int* tri_offset;         /* [n_obj + 1] */
    const double* scale;           /* [n_obj][3] */
    const double* translate;       /* [n_obj][3] */
    int n_obj;
} vpho_obj_mesh_tables;
VPHO_API int vpho_hand_obj_penetration_f64(const vpho_obj_mesh_tables* t, const float* verts, int n, int V, const double* obj_rt,
                                  const int* obj_id, double contact_thresh, double* sd, unsigned char* inside, double* per_image,
                                  void* stream);

/* The same metric for every sampled hypothesis (--eval_best with --eval_physics), appended within ABI version 13.
 * vpho_obj_mesh_accel holds two conservative filters over the records of vpho_obj_mesh_tables, built on the host
 * (vpho_amd/physics_eval.py: mesh_accel), objects concatenated:
 *   parity: the 512 x 512 hash cells in VPHO_PEN_COLUMNS x VPHO_PEN_COLUMNS columns of 512 / VPHO_PEN_COLUMNS cells a side; column
 *     (X, Y) of object o lists col_tri[col_offset[o * COLUMNS^2 + Y * COLUMNS + X] .. col_offset[.. + 1]): the triangles (indices into
 *     tri, ascending) whose cell rectangle (fields 15-18) touches the column.  A point walks the list of its own cell's column and
 *     applies the cell test and the strict containment of the single-pose kernel to every entry.
 *   nearest: the triangles in Morton order of their centroids, in clusters of VPHO_PEN_CLUSTER (the last one padded with copies of
 *     its last triangle); cluster k of object o, k in [clu_offset[o], clu_offset[o + 1]), has a bounding sphere clu_sphere[k] =
 *     (centre xyz, radius) in the model frame, the radius enlarged on the host by (1 + 2^-30) and by 2^-30 of the mesh's bounding-box
 *     diagonal, and clu_geo[k][VPHO_PEN_CLUSTER][9], bit copies of fields 19-27 of its triangles.  A cluster is skipped when
 *     |p - centre| > sqrt(best) (1 + 2^-20) + radius; every other one goes through the exact distance of the single-pose kernel.
 * vpho_hand_obj_penetration_multi_f64: verts [n][S][V][3] fp32, obj_rt [n][S][3][4] fp64, obj_id [n]: hypothesis s of the hand
 * against hypothesis s of the object.  per_hyp [n][S][4] = what vpho_hand_obj_penetration_f64 gives per_image for the n*S pairs
 * (same bits; NaN for an obj_id outside [0, n_obj)); sd [n][S][V] and inside [n][S][V] are optional (NULL: nothing is written per
 * vertex) and have its bits too.  table [n][12] = one | best | mean over the S hypotheses of an image: the four values of hypothesis
 * 0; min PD, min n_inside, MAX min-sd (the least penetrating hypothesis), max contact; the four means (sums in ascending s, fp64).
 * A NaN hypothesis makes best and mean NaN.  n == 0 is a no-op.  Deterministic (max / min / count, no atomics). */
#define VPHO_PEN_COLUMNS 64
#define VPHO_PEN_CLUSTER 16
typedef struct vpho_obj_mesh_accel {
    const int* col_offset;         /* [n_obj * VPHO_PEN_COLUMNS^2 + 1] */
    const int* col_tri;            /* [col_offset[n_obj * VPHO_PEN_COLUMNS^2]] */
    const int* clu_offset;         /* [n_obj + 1] */
    const double* clu_sphere;      /* [clu_offset[n_obj]][4] */
    const double* clu_geo;         /* [clu_offset[n_obj]][VPHO_PEN_CLUSTER][9] */
} vpho_obj_mesh_accel;
VPHO_API int vpho_hand_obj_penetration_multi_f64(const vpho_obj_mesh_tables* t, const vpho_obj_mesh_accel* acc, const float* verts, int n, int S,
                                        int V, const double* obj_rt, const int* obj_id, double contact_thresh, double* per_hyp,
                                        double* sd, unsigned char* inside, double* table, void* stream);

/* Hand-object intersection volume (--eval_volume), appended within ABI version 13.  Per (hand, object pose) pair, in
 * the object's model frame: the hand mesh is the posed vertices q_v = R^T (v - t) (fp64, the arithmetic of vpho_hand_obj_penetration_f64)
 * with `faces`, ONE closed triangle list shared by all pairs ([F][3] vertex indices in [0, V); vpho_amd/physics_eval.py: hand_faces);
 * the object is a SOLID point set: the centres of the cells of a lattice of pitch h over the object's mesh bbox that lie inside the object
 * (fp32, objects concatenated; physics_eval.solid_lattice + the single-pose kernel at identity pose).  inside_hand(c) is the z-ray
 * parity rule above applied to the posed hand mesh in ITS OWN hash frame (bbox of the q_v by min / max, scale = 511 / (max - min),
 * translate = 0.5 - scale * min, the 19 parity fields per face in the order of operations of physics_eval.mesh_tables).
 * out [n][2] = n_cells (the number of solid centres of the pair's object inside the hand, an integer) | IV = ((h * h) * h) * n_cells, one
 * fp64 product (m^3).  flags (optional, NULL: nothing is written per centre) [n][solids->max_pts] = 0 / 1 per centre of the pair's object
 * (0 behind its last centre).  An obj_id outside [0, n_obj), which cannot be refused without a host sync, or a hand vertex that is not a
 * finite number gives NaN in both columns and flags = 0.  workspace: vpho_hand_obj_intersection_workspace_bytes(n, F) bytes (-1 on a bad
 * argument): [n][F][VPHO_VOL_TRI_STRIDE] fp64 records + [n][6] fp64 scale | translate + [n][2] int (count | bad mesh).  V, F and n are free;
 * F == 0, pitch <= 0 or a face index outside [0, V) (checked on the device: NaN rows) are errors; n == 0 is a no-op.  Deterministic
 * (min / max and integer adds only). */
#define VPHO_VOL_TRI_STRIDE 19
typedef struct vpho_obj_solids {
    const float* pts;              /* [pt_offset[n_obj]][3] */
    const int* pt_offset;          /* [n_obj + 1] */
    int n_obj, max_pts;            /* max_pts = the largest per-object number of centres */
} vpho_obj_solids;
VPHO_API long long vpho_hand_obj_intersection_workspace_bytes(int n, int F);
VPHO_API int vpho_hand_obj_intersection_f64(const vpho_obj_mesh_tables* t, const vpho_obj_solids* solids, const int* faces, int F, const float* verts,
                                   int n, int V, const double* obj_rt, const int* obj_id, double pitch, double* out, unsigned char* flags,
                                   void* workspace, long long workspace_bytes, void* stream);
/* The intersection volume of EVERY sampled hypothesis (--eval_best with --eval_volume), appended within ABI version 13: verts
 * [n][S][V][3] fp32, obj_rt [n][S][3][4] fp64, obj_id [n]: hypothesis s of the hand against hypothesis s of the object.
 * per_hyp [n][S][2] = n_cells | IV, the bits vpho_hand_obj_intersection_f64 gives in `out` for the n*S pairs (NaN for an obj_id outside
 * [0, n_obj), for the whole image, and for a hypothesis with a non-finite hand vertex or a face index outside [0, V)); flags (optional)
 * [n][S][solids->max_pts] has its bits too.  table [n][6] = one_IV, one_cells (hypothesis 0) | best_IV, best_cells (the minima over S) |
 * mean_IV, mean_cells: mean_cells = (the exact integer sum of the cell counts) / S, mean_IV = ((h * h) * h) * mean_cells; a NaN
 * hypothesis makes best and mean NaN.  The kernel walks lattice COLUMNS: vpho_obj_solid_columns names the runs of solids->pts that share
 * x and y (the solid keeps lattice order, z fastest; vpho_amd/physics_eval.py: solid_columns); the part of the parity rule that depends
 * on (x, y) and the face only runs once per column.  One workgroup per pair on grid.x: n * S <= 2147483647; V, F and the solids are
 * free.  The face records are built in LDS per workgroup: vpho_hand_obj_intersection_multi_workspace_bytes is 0 (-1 on a bad argument)
 * and workspace may be NULL.  S < 1, F <= 0 and pitch <= 0 are errors; n == 0 is a no-op.  Deterministic (min / max and integer adds). */
typedef struct vpho_obj_solid_columns {
    const int* col_start;    /* [col_offset[n_obj] + 1]: index into vpho_obj_solids.pts of each non-empty lattice column's first centre,
                                columns in lattice order (i, then j), objects concatenated; a column ends where the next starts */
    const int* col_offset;   /* [n_obj + 1] */
    int n_obj, max_cols;
} vpho_obj_solid_columns;
VPHO_API long long vpho_hand_obj_intersection_multi_workspace_bytes(int n, int S, int F);
VPHO_API int vpho_hand_obj_intersection_multi_f64(const vpho_obj_mesh_tables* t, const vpho_obj_solids* solids, const vpho_obj_solid_columns* cols,
        const int* faces, int F, const float* verts /* [n][S][V][3] */, int n, int S, int V, const double* obj_rt /* [n][S][3][4] */,
        const int* obj_id /* [n] */, double pitch, double* per_hyp /* [n][S][2] */, double* table /* [n][6] */,
        unsigned char* flags /* NULL or [n][S][max_pts] */, void* workspace, long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Pseudo-force label optimisation (force_optim.py / lib/engine/force_optimization.py:110-207).
 * vpho_anchor_frames_f32: ForceAnchor.__call__ (lib/utils/physics_fn.py:224-257) -> pts [n][32][3], frames [n][32][3][3]
 * (frame[j][i] = component j of axis i), computed ONCE (the reference recomputes them in each of its 3000 iterations).
 * vpho_force_optimize_f32: the whole AdamW loop (two optimisers: `phase1_iters` steps on the cone weights against the
 * gravity-alignment loss, then scale+weights against force-balance + moment + contact-distribution losses) as one
 * persistent workgroup per batch of B <= 64 samples (the batch-mean force loss couples the samples of a batch, :146).
 * Inputs are laid out [n_batches*B]...; gravity/com [..][3] in the flipped (right-hand) frame; outputs force_local /
 * force_global [..][32][3] (zero where !is_grasped, :199-202), final scale [..][32], weight [..][32][8],
 * losses [n_batches][4] = (force, gravity, moment, distribution) of the last iteration. */
VPHO_API int vpho_anchor_frames_f32(const vpho_anchor_tables* t, const float* verts, long long n_hands, float* pts, float* frames, void* stream);
VPHO_API int vpho_force_optimize_f32(const float* pts, const float* frames, const float* gravity, const float* com, const float* force_contact,
                            const unsigned char* is_grasped, int n_batches, int B, int iters, int phase1_iters, float lr,
                            float* force_local, float* force_global, float* scale, float* weight, float* losses, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Hand-object contact detection (lib/utils/physics_fn.py:47-117,201-221; caller
 * lib/dataset/base.py:841-912).  vpho_contact_detect_f32 is one direction of detect_hand_and_object_contact: for each of
 * n samples, every query point (with unit normal) finds its nearest target point, gates on the signed distance along the
 * normal in (normal_lo, normal_hi) and the tangential distance < vertical_thresh, and gets the double-sigmoid weight
 * normalised to 1 at distance 0; nn_index (optional) = nearest target index where in contact, else -1.  Call it hand->object
 * for hand_contact_map and object->hand for obj_contact_map / obj_contact_to_hand_vert.
 * vpho_force_contact_f32 pools a hand contact map (rows of `ld` >= 778 floats) onto the 32 CPF anchors and applies the
 * check_is_grasped rule. */
VPHO_API int vpho_contact_detect_f32(const float* query, const float* query_normals, const float* target, int n, int n_query, int n_target,
                            float normal_lo, float normal_hi, float vertical_thresh, float decay_lo, float decay_hi,
                            float* weight, int* nn_index, void* stream);
VPHO_API int vpho_force_contact_f32(const vpho_anchor_tables* t, const float* hand_contact, int ld, int n, float thresh,
                           float* force_contact, unsigned char* is_grasped, void* stream);
/* The front of that chain (appended within ABI version 13): vertex normals of the posed hand mesh and the finger-gap fill, one
 * workgroup per sample.  Replaces lib/dataset/base.py:887-891 (trimesh.Trimesh(hand_verts, hand_faces).vertex_normals, n / (|n| + 1e-20),
 * the fill, n / (|n| + 1e-20) again) and lib/utils/hand_fn.py:294-384 (fill_finger_gaps_in_mano, 778 -> 1080 rows).
 * Table (device arrays, built and VALIDATED once per mesh by the caller; the kernel trusts every index): faces [F][3]; the incidence list
 * vertex -> (face, corner) in CSR form, csr_offset [V + 1], csr_entry [3 F] = face * 4 + corner with the faces of a vertex in ascending
 * index; links [L][2] and alpha [L] (fp64) of the gap fill.  V in 1 .. 1024, F <= 2048, L <= 1024, larger sizes are refused.
 * verts [n][V][3] -> verts_filled, normals_filled [n][V + L][3].
 * Normals (a restatement of trimesh's angle-weighted vertex normals): face normal = cross(v1 - v0, v2 - v0) unitised, a face whose cross
 * product is exactly zero contributes nothing; corner angle = acos(clamp(u . w, -1, 1)) of the two unit edge vectors leaving the corner;
 * vertex normal = sum over csr_entry of angle * face normal, unitised (the zero vector when the sum is zero: an unreferenced vertex,
 * cancelling faces), then n / (|n| + 1e-20).  Rows V + l of both outputs = alpha[l] * x[links[l][0]] + (1 - alpha[l]) * x[links[l][1]];
 * every normal row is then divided by (|n| + 1e-20) once more.  fp64 from the fp32 input, each output rounded to fp32 once; fixed
 * summation order, no atomics: bit-reproducible.  A NaN coordinate reaches its faces, the normals of their vertices and the links
 * through either; every other value stays finite.  n == 0: success without a launch. */
typedef struct {
    const int* faces; const int* csr_offset; const int* csr_entry; const int* links; const double* alpha;
    int V, F, L;
} vpho_hand_surface_table;
VPHO_API int vpho_hand_surface_f32(const vpho_hand_surface_table* t, const float* verts, int n, float* verts_filled, float* normals_filled,
                          void* stream);
/* The hand contact map of EVERY sampled hypothesis and its agreement with the annotation's (--eval_grasp), appended
 * within ABI version 13.  vpho_contact_multi_f32 is the hand -> object direction of vpho_contact_detect_f32 for n * S (hand hypothesis s,
 * object hypothesis s) pairs in the object's MODEL frame: no posed object vertex is written, and the nearest vertex comes from a pruned
 * walk that returns the index of the scan of all vertices (csrc/contact_multi.hip has the argument).
 * vpho_obj_vertex_accel (built on the host, vpho_amd/grasp_eval.py: vertex_accel), objects concatenated, none padded: vert, the FULL
 * vertices of every object in Morton order (fp64, model frame), index, each one's ORIGINAL index within its object; object o owns the
 * clusters [clu_offset[o], clu_offset[o + 1]), cluster k the rows [clu_start[k], clu_start[k + 1]) of vert / index (32 rows, fewer in
 * an object's last cluster; the kernel takes any tiling), clu_sphere[k] = (centre xyz, radius): the centre of the rows' bounding box and
 * their largest distance from it, enlarged on the host by (1 + 2^-30) and by 2^-30 of the object's bounding-box diagonal.
 * hand_verts, hand_normals [n][S][Nh][3] fp32: the filled hand surface of vpho_hand_surface_f32 in ITS frame (flipped to a right hand,
 * relative to the root joint); root [n][3] fp64, is_right [n], obj_rt [n][S][3][4] fp64 [R | t] (model -> camera), obj_id [n].  All in
 * fp64: c = (sg h_x, h_y, h_z) + root with sg = +1 / -1 for a right / left hand, p = R^T (c - t), m = R^T (sg n_x, n_y, n_z); v* = the
 * vertex with the smallest |p - v|^2, the smaller original index on an exact tie; nd = (p - v*) . m, vd = |(p - v*) - nd m|; contact iff
 * normal_lo < nd < normal_hi and vd < vertical_thresh (the fp32 gates widened to fp64).  weight [n][S][Nh] = the double-sigmoid weight of
 * vpho_contact_detect_f32 at nd, over its value at 0, clamped to [0, 1], rounded to fp32; 0 without contact.  nn_index (optional)
 * [n][S][Nh] = v*'s original index where in contact, else -1; nd, vd (optional) [n][S][Nh] fp64, of every vertex.  A pair with a
 * non-finite pose, root, hand vertex or normal, an obj_id outside [0, n_obj) or an object without vertices: NaN in weight, nd and vd and
 * -1 in nn_index for the whole pair, nothing out of bounds is read.  One workgroup per pair on grid.x: n * S <= 2147483647.  The
 * thresholds must satisfy normal_lo < decay_lo < decay_hi < normal_hi; n == 0 is a no-op.  Deterministic.
 * vpho_contact_agreement_f32: weight [n][S][Nh] against weight_gt [n][Nh], with c = weight > 0 and g = weight_gt > 0; force_contact
 * [n][S][32] / is_grasped [n][S] (vpho_force_contact_f32 over the n * S maps) against force_contact_gt [n][32] / is_grasped_gt [n].
 * counts [n][S][3] = TP, P, G (|c & g|, |c|, |g|); values [n][S][8] fp64 = IoU = TP / (P + G - TP), precision = TP / P, recall = TP / G,
 * F1 = 2 TP / (P + G) (each NaN when its denominator is 0), MAE = mean |weight - weight_gt| over Nh, anchor_agree = the share of the 32
 * anchors with equal (force_contact > 0), grasped = is_grasped, grasp_agree = (is_grasped == is_grasped_gt).  A pair with a NaN in either
 * map: NaN values, zero counts.  table [n][24] = the values of hypothesis 0 | best-of-S (each value's maximum on its own, MAE's minimum)
 * | mean-of-S (sum in ascending s over how many), both over the hypotheses where the value is not NaN, NaN where it never is.
 * n == 0 is a no-op.  Deterministic (fixed summation order, no atomics). */
typedef struct vpho_obj_vertex_accel {
    const double* vert;            /* [clu_start[clu_offset[n_obj]]][3] */
    const int* index;              /* [clu_start[clu_offset[n_obj]]] */
    const int* clu_offset;         /* [n_obj + 1] */
    const int* clu_start;          /* [clu_offset[n_obj] + 1] */
    const double* clu_sphere;      /* [clu_offset[n_obj]][4] */
    int n_obj;
} vpho_obj_vertex_accel;
VPHO_API int vpho_contact_multi_f32(const vpho_obj_vertex_accel* acc, const float* hand_verts, const float* hand_normals, int n, int S, int Nh,
                           const double* root, const unsigned char* is_right, const double* obj_rt, const int* obj_id,
                           float normal_lo, float normal_hi, float vertical_thresh, float decay_lo, float decay_hi,
                           float* weight, int* nn_index, double* nd, double* vd, void* stream);
VPHO_API int vpho_contact_agreement_f32(const float* weight, const float* weight_gt, const float* force_contact, const unsigned char* is_grasped,
                               const float* force_contact_gt, const unsigned char* is_grasped_gt, int n, int S, int Nh,
                               int* counts, double* values, double* table, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training of the score networks (first slice): the denoising-score-matching step of
 * ScoreBasedModelAgent.get_score_loss / loss_fn (lib/model/score_based_model.py:11-42,117-128) on BaseDenoiser
 * (lib/model/denoiser.py:68-82) -- forward with saved activations, analytic backward to every denoiser parameter and to the
 * image encoding, AdamW (lib/engine/train_diff_hand_obj.py:49-52).  rows = repeat_num * batch, row r = rep * batch + b.
 * The GEMMs run through vpho_conv2d_nhwc_f32 (1x1 convolutions on [rows][C] matrices); these are the pieces around them. */
/* std = 0.01 * 5000^t (sde.py:15-18), x_t = gt_pose[b] + z * std zero-padded to Dp columns, emb = [sin, cos](t W 2 pi)
 * (denoiser.py:29-31).  t [rows], z [rows][D], fourier_W [64] -> x_t [rows][Dp], emb [rows][128], std_out [rows] */
VPHO_API int vpho_dsm_prepare_f32(const float* gt_pose, const float* t, const float* z, const float* fourier_W, int bs, int reps, int D, int Dp,
                         float* x_t, float* emb, float* std_out, void* stream);
/* second ParallelLinear (256 -> 3 per head, parallel_linear.py:27-35) + division by (std + 1e-7) (denoiser.py:80-81):
 * h [rows][nheads*256], w2 [nheads][256][3], b2 [nheads][3] -> score [rows][3*nheads] */
VPHO_API int vpho_plinear2_fwd_f32(const float* h, const float* w2, const float* b2, const float* std_rows, long long rows, int nheads,
                          float* score, void* stream);
/* loss = mean over batch*reps of sum_d std^2 (score - target)^2, target = -z std / std^2 (score_based_model.py:33-41);
 * dout = d loss / d (un-normalised head output) [rows][D]; loss: one double on the device; partial_ws: >= 1024 doubles */
VPHO_API int vpho_dsm_loss_f32(const float* score, const float* z, const float* std_rows, long long rows, int D, int batch_times_reps,
                      float* dout, double* loss, double* partial_ws, int partial_cap, void* stream);
/* Weight gradient of an NHWC convolution without materialised im2col / transposes (torch.nn.functional.conv2d's autograd for
 * every nn.Conv2d of lib/model/backbone_FPN_HFL.py, encoding.py, head_inplane.py under lib/engine/train_diff_hand_obj.py:181-182):
 * dw[co][(r*KW+s)*Cin + ci] = sum_{n,oy,ox} dy[n,oy,ox,co] * x[n, oy*stride+r-pad_y, ox*stride+s-pad_x, ci]   (zero outside the image)
 * in the packed layout of the forward weights.  x [N][H][W][x_ld], dy [N][OH][OW][dy_ld]; Cin, Cout and both leading dimensions
 * multiples of 4, pointers 16-byte aligned.  The pixel range is reduced in slices (fp32 MFMA accumulation inside a slice, slices
 * added in ascending order): workspace of vpho_conv2d_wgrad_workspace_bytes(...) bytes (may be 0 -> workspace may be NULL). */
VPHO_API long long vpho_conv2d_wgrad_workspace_bytes(int N, int OH, int OW, int Cin, int Cout, int KH, int KW);
VPHO_API int vpho_conv2d_wgrad_nhwc_f32(const float* x, int N, int H, int W, int Cin, int x_ld, const float* dy, int OH, int OW, int Cout, int dy_ld,
                               int KH, int KW, int stride, int pad_y, int pad_x, float* dw, void* workspace, void* stream);
/* The same weight gradient when dY is known to be zero outside RoI windows (the gradient of a map that is only read through RoIAlign:
 * the FPN smoothing convolutions, VPHO.py:126-129): the reduction runs over the ascending list of live 32-pixel groups that
 * vpho_window_groups_i32 builds on the device from the window table of vpho_roi_windows_i32 (a group is live when one of its pixels
 * lies in its image's window); the pixel slices cut the list instead of the pixel range.  Needs OW % 32 == 0.  Same workspace. */
VPHO_API int vpho_window_groups_i32(const int* wins, int N, int H, int W, int* group_list, int* group_count, void* stream);
VPHO_API int vpho_conv2d_wgrad_groups_nhwc_f32(const float* x, int N, int H, int W, int Cin, int x_ld, const float* dy, int OH, int OW, int Cout,
                                      int dy_ld, int KH, int KW, int stride, int pad_y, int pad_x, const int* group_list,
                                      const int* group_count, float* dw, void* workspace, void* stream);
/* Training-mode tail of HeadMano for one batch of hands (lib/model/head_mano.py:60-87 forward + get_hand_verts, :89-133 get_loss,
 * weights applied as lib/model/VPHO.py:214-219): rot6d [bs][96] (fc_pose output) -> rotation_6d_to_matrix -> ManoLayer -> root-centred
 * vertices / joints in metres (optional outputs verts [bs][778][3], joints [bs][21][3], may be NULL); the four losses against
 * gt_vert / gt_joint / gt_rot6d (= mano_aa_to_6D(gt pose)[:96]) / gt_shape (right hands only, is_right [bs]) and the gradient of
 * w_vert*vert_loss + w_joint*joint_loss + w_pose*mano_pose_loss + w_shape*mano_shape_loss w.r.t. rot6d and shape.
 * loss_parts [bs][4]: per-hand sums of squared differences (vert, joint, pose, shape) in fp64 -- the caller applies
 * weight / (bs * 2334 | bs * 63 | bs * 96 | bs * 10).  is_ho3d (per hand, optional): the regressed joints of those hands enter the joint
 * loss in HO3D's convention (get_joint_aligned_with_HO3D, VPHO.py:154-157, hand_fn.py:454-461: joints re-ordered, HO3D's own tip vertices).
 * A batch without any right hand gives a shape loss of 0 here (the reference takes the mean of an empty tensor: NaN). */
VPHO_API int vpho_mano_train_f32(const vpho_mano_tables* t, const float* rot6d, const float* shape, const float* gt_vert, const float* gt_joint,
                        const float* gt_rot6d, const float* gt_shape, const unsigned char* is_right, const unsigned char* is_ho3d, int bs,
                        float w_vert, float w_joint, float w_pose, float w_shape,
                        float* d_rot6d, float* d_shape, double* loss_parts, float* verts, float* joints, void* stream);
/* JointsMSELoss (lib/model/head_inplane.py:191-203: nn.MSELoss, mean over all elements) times its loss weight
 * (VPHO.py:214-219): loss[0] = weight * mean((pd - gt)^2) in fp64, grad = weight * 2 (pd - gt) / n.  partial_ws: >= partial_cap doubles */
VPHO_API int vpho_mse_loss_f32(const float* pd, const float* gt, long long n, float weight, float* grad, double* loss, double* partial_ws, int partial_cap,
                      void* stream);
/* backward of the second ParallelLinear and of the ReLU in front of it: dpre [rows][nheads*256] (gradient at the first
 * layer's pre-activation), dw2 [nheads][256][3], db2 [nheads][3] */
VPHO_API int vpho_plinear2_bwd_f32(const float* h, const float* dout, const float* w2, long long rows, int nheads, float* dpre, float* dw2, float* db2,
                          void* stream);
/* dx = y > 0 ? dy : 0 on [rows][cols] slices with leading dimensions (gradient through nn.ReLU given its output y) */
VPHO_API int vpho_relu_bwd_f32(const float* dy, int ld_dy, const float* y, int ld_y, long long rows, int cols, float* dx, int ld_dx, void* stream);
/* out[c] = sum_r x[r][c] (bias gradients; fp64 partial sums over row chunks, combined in a fixed order).
 * workspace: vpho_bn_workspace_bytes(cols) bytes */
VPHO_API int vpho_colsum_f32(const float* x, int ld, long long rows, int cols, float* out, void* workspace, void* stream);
/* out[b][c] = sum_rep x[rep*bs + b][c_off + c]: the encoding is shared by the repeat_num draws of an image */
VPHO_API int vpho_sum_repeats_f32(const float* x, int ld, int c_off, int bs, int reps, int cols, float* out, void* stream);
/* y[c][r] = x[r][c] (operands of the weight-gradient GEMMs) */
VPHO_API int vpho_transpose_f32(const float* x, int rows, int cols, int ldx, float* y, int ldy, void* stream);
/* Transposed im2col, the second operand of a convolution's weight gradient dW[co][(r,s,ci)] = sum_p dY^T[co][p] * out[(r,s,ci)][p]
 * (the product itself is vpho_conv2d_nhwc_f32 as a GEMM): out[(r*KW+s)*Cin + ci][p] = x[n, oy*stride+r-pad_y, ox*stride+s-pad_x, ci],
 * p = (n*OH+oy)*OW+ox, zero outside the image and in the padding columns p >= N*OH*OW of the leading dimension ldo. */
VPHO_API int vpho_im2col_t_f32(const float* x, int N, int H, int W, int Cin, int x_ld, int KH, int KW, int stride, int pad_y, int pad_x,
                      int OH, int OW, float* out, long long ldo, void* stream);
/* nn.BatchNorm2d in training mode on NHWC rows (rows = N*H*W, leading dimension ld >= C) -- every BatchNorm of
 * backbone_FPN_HFL.py / encoding.py / head_inplane.py under model.train() (train_diff_hand_obj.py:171): batch mean and biased
 * variance (fp64 two-level reduction), y = lrelu((x - mean) * invstd * gamma + beta, slope) (slope 1 = no activation), running
 * statistics updated with `momentum` and the unbiased variance; save_mean / save_invstd feed the backward:
 * dbeta = sum dy, dgamma = sum dy * xhat, dx = gamma * invstd / rows * (rows * dy - dbeta - xhat * dgamma).
 * (For a fused activation pass its backward first: vpho_lrelu_bwd_f32 on y.)  res (may be NULL; ABI version 4): the residual
 * branch of a bottleneck, y = lrelu(bn(x) + res, slope) (Bottleneck.forward, backbone_FPN_HFL.py:347-349); its gradient is the
 * gradient of the sum.  workspace: vpho_bn_workspace_bytes(C). */
VPHO_API long long vpho_bn_workspace_bytes(int C);
VPHO_API int vpho_bn_train_forward_f32(const float* x, long long rows, int C, int ld, const float* gamma, const float* beta, float eps, float momentum,
                              float slope, float* running_mean, float* running_var, float* save_mean, float* save_invstd, const float* res,
                              float* y, void* workspace, void* stream);
VPHO_API int vpho_bn_train_backward_f32(const float* x, const float* dy, long long rows, int C, int ld, const float* gamma, const float* save_mean,
                               const float* save_invstd, float* dx, float* dgamma, float* dbeta, void* workspace, void* stream);
/* The same two calls when the reductions were taken by the producing convolution's epilogue (ABI version 13; vpho_conv_desc.stats,
 * vpho_conv3x3_winograd_stats_nhwc_f32): stats = [stats_rows][6][C] float partial rows (forward: sum x | sum x^2 | pivot |
 * sum (x - pivot) | sum (x - pivot)^2 | count, planes 2 .. 5 merged about one pivot per channel; backward: sum dy | sum dy * xhat in planes 0, 1), combined here in
 * fp64 in a fixed order -- the pass over x (and dy) that vpho_bn_train_*_f32 start with is not run.  Everything else as above. */
VPHO_API int vpho_bn_train_forward_stats_f32(const float* x, long long rows, int C, int ld, const float* stats, int stats_rows, const float* gamma,
                                    const float* beta, float eps, float momentum, float slope, float* running_mean, float* running_var,
                                    float* save_mean, float* save_invstd, const float* res, float* y, void* workspace, void* stream);
/* backward: stats may be NULL (stats_rows 0: the call takes its own reduction pass).  res (may be NULL): the other branch of a residual sum,
 * added to dx (encoding.Residual's identity shortcut, encoding.py:21-36: d input = BatchNorm backward + d shortcut).  dx_colsum (may be NULL;
 * C floats): the column sums of the dx it stores = the bias gradient of the convolution that produced x, taken while dx is written. */
VPHO_API int vpho_bn_train_backward_stats_f32(const float* x, const float* dy, long long rows, int C, int ld, const float* gamma, const float* save_mean,
                                     const float* save_invstd, const float* stats, int stats_rows, const float* res, float* dx, float* dgamma,
                                     float* dbeta, float* dx_colsum, void* workspace, void* stream);
/* dx = y > 0 ? dy : dy * slope: backward of nn.LeakyReLU(slope) / nn.ReLU (slope 0) given its OUTPUT y */
VPHO_API int vpho_lrelu_bwd_f32(const float* dy, const float* y, long long n, float slope, float* dx, void* stream);
/* nn.MaxPool2d backward (backbone_FPN_HFL.py:209): dx[n,iy,ix,c] = sum of dy over the windows whose first maximum (row-major)
 * is (iy,ix); x is the pooling input.  Deterministic gather, no atomics. */
VPHO_API int vpho_maxpool_bwd_nhwc_f32(const float* x, const float* dy, int N, int H, int W, int C, int k, int stride, int pad, float* dx, void* stream);
/* the same with a byte workspace (vpho_maxpool_bwd_workspace_bytes; 0 = not needed) for overlapping windows: arg-max position of
 * every window first, then the gather compares position codes instead of re-scanning windows (bit-identical results) */
VPHO_API long long vpho_maxpool_bwd_workspace_bytes(int N, int H, int W, int C, int k, int stride, int pad);
VPHO_API int vpho_maxpool_bwd_ws_nhwc_f32(const float* x, const float* dy, int N, int H, int W, int C, int k, int stride, int pad, float* dx,
                                 void* workspace, void* stream);
/* F.interpolate(mode='bilinear', align_corners=False) backward (FPN._upsample_add, backbone_FPN_HFL.py:66-68):
 * dy [N][OH][OW][C] -> dx [N][H][W][C] */
VPHO_API int vpho_resize_bilinear_bwd_nhwc_f32(const float* dy, int N, int OH, int OW, int C, int H, int W, float* dx, void* stream);
/* torchvision.ops.roi_align backward (VPHO.py:125-128 under loss.backward()): dy [N][P][P][ldo] (channel slice c_off..c_off+C, optionally
 * W-flipped like the forward) accumulated into dfeat [N][H][W][C] (+=; zero-initialise it, or pass another gradient of the same
 * map to sum both).  One RoI per image (box n belongs to image n).  Channel counts / strides that are multiples of 4 take a gather
 * with a fixed summation order (each feature pixel sums the few bins that reach it); other shapes scatter with fp32 atomics. */
VPHO_API int vpho_roi_align_bwd_nhwc_f32(const float* dy, int ldo, int c_off, int N, int H, int W, int C, const float* boxes, float spatial_scale,
                                int out_size, const unsigned char* flip_w, float* dfeat, void* stream);
/* backward of vpho_align_heatmap_nhwc_f32 (align_hm_to_bbox_rectangle + flip, VPHO.py:333-346,139): dout [N][S][S][C] -> dhm [N][S][S][C]
 * (+=: zero-initialise dhm; a gather with a fixed summation order for S <= 120, fp32 atomics beyond) */
VPHO_API int vpho_align_heatmap_bwd_nhwc_f32(const float* dout, int N, int size, int C, const float* bbox, const float* bbox_rect,
                                    const unsigned char* flip_w, float* dhm, void* stream);
/* y = lrelu(a + b, slope): `out += residual; out = leakyrelu(out)` of Bottleneck.forward (backbone_FPN_HFL.py:347-348); slope 1 = a + b */
VPHO_API int vpho_add_lrelu_f32(const float* a, const float* b, long long n, float slope, float* y, void* stream);
/* torch.optim.AdamW single-tensor step (decoupled weight decay, bias-corrected moments); grad_scale multiplies the gradient
 * first (1 / world_size after a sum all-reduce) */
VPHO_API int vpho_adamw_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, float grad_scale, void* stream);
/* the same step for a list of tensors in one launch.  segments: device array of n_segments records
 * { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; long long n; long long first_block; } with
 * first_block = running sum of ceil(n / 1024) over the preceding records, total_blocks = that sum over all records. */
VPHO_API int vpho_adamw_multi_f32(const void* segments, int n_segments, long long total_blocks, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, float grad_scale, void* stream);
/* ---- optimiser tail (optim.hip): global gradient norm + Adam / AdamW with the clip coefficient formed on the device ------------------
 * sum of grad[i]^2 over a contiguous fp32 buffer (any 4-byte alignment) into ONE fp64 value on the device.  fp64 accumulation in a
 * fixed order (a grid that depends on n alone, contiguous chunks, lanes then waves, then the partials in ascending index; no atomics):
 * two runs, and data-parallel replicas holding the same gradients, get the same bits.  workspace: vpho_grad_sqnorm_workspace_bytes(n)
 * bytes, 8-byte aligned (-1 = bad argument). */
VPHO_API long long vpho_grad_sqnorm_workspace_bytes(long long n);
VPHO_API int vpho_grad_sqnorm_f64(const float* grad, long long n, double* out, void* workspace, void* stream);
/* vpho_adamw_multi_f32's segment table and block ownership, plus: kind 0 = torch.optim.AdamW (decoupled decay; with sqnorm NULL the
 * bits of vpho_adamw_multi_f32), kind 1 = torch.optim.Adam with L2 decay (g += weight_decay * param before the moments).  sqnorm
 * (device, may be NULL) = the sum of squares of the SUMMED gradient: every thread forms torch.nn.utils.clip_grad_norm_'s
 * coef = min(1, max_norm / (grad_scale * sqrt(*sqnorm) + 1e-6)) in fp64, rounds it once to fp32 and steps with (g * grad_scale) * coef;
 * coef == 1 leaves the bits of the unclipped step, a non-finite norm makes the update NaN as torch does.  grad_scale =
 * 1 / (world_size * accumulation_steps).  The gradients are only read. */
VPHO_API int vpho_optim_multi_f32(const void* segments, int n_segments, long long total_blocks, int kind, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, float grad_scale, const double* sqnorm, float max_norm, void* stream);
/* ---- moving average of the weights (ema.hip): ExponentialMovingAverage.update (lib/model/ema.py:25-44) for a list of tensors in one
 * launch.  table: device array of n_tensors records { const float* param; float* shadow; long long n; long long first_block; } with
 * first_block = running sum of ceil(n / 1024) over the preceding records, blocks = that sum over all records (the scheme of
 * vpho_optim_multi_f32).  shadow -= one_minus_decay * (shadow - param) as torch evaluates it: three fp32 operations, each rounded
 * once, never contracted; NaN and infinities propagate.  The caller forms one_minus_decay = 1 - min(decay, (1 + k) / (10 + k)) in
 * double (k = number of updates, this one included) and rounds it once.  param is only read.  n_tensors == 0 (or blocks == 0): success
 * without a launch; a negative count or a NULL table with n_tensors > 0: bad argument. */
VPHO_API int vpho_ema_multi_f32(const void* table, int n_tensors, long long blocks, float one_minus_decay, void* stream);
/* ---- frames in (frames.hip): the per-image work of the reference's Dataset.__getitem__, lib/dataset/dexycb6.py:339-469 -------------
 * vpho_frame_patch_f32: frames (n,H,W,3) uint8 -> out (n,3,P,P) fp32, the `rgb` of the batch schema.  Replaces cv2.warpAffine(rgb,
 * rotmat_2d[:2], (P,P), INTER_CUBIC) (dexycb6.py:345), the RGB shift / brightness / saturation of image_augmentor.run_color (:389-391,
 * base.py:381-382), the left-hand mirror rgb_patch[:, ::-1] (:398-399), normalize_rgb (:442, base.py:97-102) and timm's RandomErasing
 * mode 'pixel' (:444).  minv (n,6) fp64: rows 0-1 of the INVERSE of rotmat_2d, patch (x, y, 1) -> frame; the coordinate, its floor and
 * fraction are fp64, the Keys weights (A = -0.75, taps floor-1 .. floor+2, outside the frame 0) and the sums fp32, rows first; the sum is
 * rounded to nearest (ties to even) and clamped to [0, 255].  OpenCV's 1/32-pixel coordinate grid and 15-bit weights are NOT reproduced.
 * colour (n,5) fp32 or NULL: dr, dg, db, brightness b, saturation s -- v + d, then v * b, then s * v + (1 - s) * gray with gray =
 * round(0.299 R + 0.587 G + 0.114 B); every stage ends rounded and clamped.  flip (n) uint8 or NULL: non-zero writes patch column x at
 * P - 1 - x.  Then (v / 255 - mean) / std in three fp32 operations (ImageNet mean / std).  erase (n,4,4) int32 or NULL: up to four
 * rectangles x0, y0, x1, y1 (half open, OUTPUT coordinates, x1 <= x0 = none) filled with N(0,1): Philox4x32-10, counter (y * P + x, 0, 0,
 * 0), key (n,2) uint32; a word's upper 23 bits give u = (k + 0.5) / 2^23; (w0, w1) and (w2, w3) are two Box-Muller pairs
 * sqrt(-2 ln u1) (cos, sin)(2 pi u2); channels 0, 1, 2 take cos, sin of the first pair and cos of the second.  n == 0: success
 * without a launch.  frames are only read. */
VPHO_API int vpho_frame_patch_f32(const unsigned char* frames, int n, int H, int W, const double* minv, const float* colour, const unsigned char* flip,
                         const int* erase, const unsigned int* key, int P, float* out, void* stream);
/* vpho_heatmap_targets_f32: out (n,J,S,S) fp32 heat-map targets of lib/utils/misc_fn.py:285-385, no intermediate map.  pts (n,J,2) fp64
 * patch coordinates; g (G,G) fp32: the reference's Gaussian table rounded to fp32 (what it stores into its fp32 map); sigma as the
 * generator holds it.  adaptive == 0, HeatmapGenerator.get_heatmap (:324-330, :297-322): box (n,4) fp64 = x0, y0, max_wh, unused;
 * p = (pt - box[:2]) / max_wh * (S - 1), + 1 in x where left (n) uint8 (NULL: nowhere) is non-zero; truncated toward zero, a joint outside
 * [0,S) gives a zero map; the table lies with its corner at rint(x - 3 sigma - 1) (ties to even, as np.round), up to rint(x + 3 sigma + 2),
 * clipped to the map.  adaptive != 0, AdaptiveHeatmapGenerator.__call__ (:372-385): box = x0, y0, w, h; res (n,2) int32 = the tight map's
 * width and height (>= 1: the caller checks); p = (pt - box[:2]) * res / (w, h) in that order; the tight map's stamp is evaluated at the
 * four taps of a half-pixel-centre bilinear resize to S x S (source (d + 0.5) * res / S - 0.5, taps clamped to the edge: the convention of
 * cv2.resize INTER_LINEAR), weights and sums fp32; values below gmin (the table's fp64 minimum) become 0.  n == 0: no launch. */
VPHO_API int vpho_heatmap_targets_f32(const double* pts, const double* box, const int* res, const unsigned char* left, const float* g, int G, double sigma,
                             double gmin, int n, int J, int S, int adaptive, float* out, void* stream);
/* ---- photometric augmentation (photo.hip, ABI version 14): the transforms of the reference's ImageAugmentor
 * (lib/dataset/base.py:349-397) that need a per-image statistic or a neighbourhood -- A.CLAHE, the contrast and hue of A.ColorJitter,
 * A.AdvancedBlur, A.MotionBlur -- as this project's own rules (no parity with albumentations or OpenCV is claimed).
 * Every stage ends on an integer grey level: the image between two stages is `levels` (n,P,P,3) uint8.  n <= 65535, P <= 16384; n == 0:
 * success without a launch.  Stages in the reference's order, on the UNMIRRORED patch: levels, CLAHE, colour, filter (which mirrors last).
 * vpho_photo_levels_u8: the bicubic crop of vpho_frame_patch_f32 (same minv, same arithmetic) before any colour stage, not mirrored.
 * vpho_photo_clahe_lut_u8 (P % 8 == 0, an 8 x 8 grid of tiles of tw = P / 8 pixels a side): clip (n) int32, 0 = the sample's gate is off
 * (nothing is written for it), else the clip count max(1, int(clip_limit * tw * tw / 256)) formed by the caller.  l8 (n,P,P): rint(L * 255
 * / 100) of CIE Lab in fp64 (sRGB linearisation 0.04045 / 12.92 / 2.4, the D65 matrix, white (0.950456, 1, 1.088754), f(t) = cbrt(t) above
 * 0.008856, else 7.787 t + 16 / 116).  lut (n,64,256), tile ty * 8 + tx, integers only: the tile's histogram of l8, counts above clip cut
 * off, excess / 256 added to every bin, the remaining r counts given one each to bins 0, step, 2 step, ... (step = max(256 / r, 1)),
 * lut[i] = 255 * cumsum[i] / (tw * tw) rounded half to even.
 * vpho_photo_clahe_apply_u8: per pixel the four LUTs around the tile coordinate (2 x + 1 - tw) / (2 tw) (tile indices clamped to 0..7),
 * bilinear as an integer numerator over 4 tw tw, rounded half to even -> l8_out (n,P,P; may be NULL); L' = l8' * 100 / 255 with the
 * pixel's own unquantised a and b back to sRGB in fp64, rounded and clamped -> out (may be levels).  A sample with clip 0 is copied.
 * vpho_photo_grey_sum_u8: sums (n) 64-bit, ZERO on entry: the sum over the image of gray = round(0.299 R + 0.587 G + 0.114 B) after the
 * shift and brightness of colour (n,5; NULL: of the levels as they are).  Integer adds only: the same bits in every run.
 * vpho_photo_colour_u8: v + d, v * b (colour, as vpho_frame_patch_f32), contrast (n) or NULL: f * v + (1 - f) * m with the integer mean
 * m = (2 sum + N) / (2 N), N = P * P, of sums; saturation (colour); hue (n) or NULL, 0 = skipped: v / 255 to HSV by torchvision's formulas,
 * h + delta - floor(h + delta), back, times 255.  All fp32, every operation rounded once, every stage rounded and clamped.  out may be levels.
 * vpho_photo_filter_f32: two filters, then the mirror, normalisation and erasing of vpho_frame_patch_f32 (flip, erase, key as there) ->
 * out (n,3,P,P) fp32.  k1, k2 (n,49) fp32: a K x K kernel, row-major, in the first K * K entries, K1, K2 (n) int32 odd in 1..7 (anything
 * else gives that sample NaN; the caller refuses it).  Each filter is the correlation sum_ky sum_kx k[ky][kx] * v[y + ky - K/2][x + kx -
 * K/2], accumulated in fp32 from 0 in that order, border reflect-101, rounded and clamped; the second reads the first's integer image. */
VPHO_API int vpho_photo_levels_u8(const unsigned char* frames, int n, int H, int W, const double* minv, int P, unsigned char* out, void* stream);
VPHO_API int vpho_photo_clahe_lut_u8(const unsigned char* levels, const int* clip, int n, int P, unsigned char* l8, unsigned char* lut, void* stream);
VPHO_API int vpho_photo_clahe_apply_u8(const unsigned char* levels, const int* clip, const unsigned char* l8, const unsigned char* lut, int n, int P,
                        unsigned char* out, unsigned char* l8_out, void* stream);
VPHO_API int vpho_photo_grey_sum_u8(const unsigned char* levels, const float* colour, int n, int P, long long* sums, void* stream);
VPHO_API int vpho_photo_colour_u8(const unsigned char* levels, const float* colour, const float* contrast, const float* hue, const long long* sums, int n,
                   int P, unsigned char* out, void* stream);
VPHO_API int vpho_photo_filter_f32(const unsigned char* levels, const float* k1, const int* K1, const float* k2, const int* K2, const unsigned char* flip,
                    const int* erase, const unsigned int* key, int n, int P, float* out, void* stream);

/* ---- predictions to pixels (raster.hip, appended within ABI version 13): a batched, deterministic triangle rasteriser and the overlay
 * compositor.  They stand in for the reference's pytorch3d renderer, lib/utils/render_fn.py, and what lib/dataset/base.py:472-500,632-688
 * does with it (get_obj_front_and_back_depth_map and the rendered overlays).  Nothing here is compared with pytorch3d: the rules below are
 * this project's own, chosen to be exact and watertight.
 * Table (device arrays, built and VALIDATED once per asset set by the caller; the kernels trust every index): the meshes' triangles
 * concatenated, faces [sum F][3] with vertex indices local to their mesh, face_offset [M + 1], vert_count [M].
 * vpho_mesh_raster_f32: n images of H x W pixels, 1 <= H, W <= 2048 (larger sizes are refused), one mesh each -- a mixed batch is ONE launch.
 * verts [n][Vmax][3] fp32, camera frame, metres; mesh_id [n]; K [n][3][3] fp64 (upper triangular, the skew entry K01 is honoured);
 * face_stride >= the face count of every mesh the batch uses (faces beyond it are not drawn); workspace of vpho_mesh_raster_bytes(n,
 * face_stride) bytes (-1 = bad argument).  Outputs [n][H][W], any of them may be NULL: depth_front / depth_back fp32 metres, 0 where nothing
 * covers the pixel; face_front / face_back int32, the face index WITHIN the mesh, -1 where nothing covers the pixel.  n == 0: success
 * without a launch.  An image whose mesh_id lies outside the table comes back empty.
 * Projection, fp64 from the fp32 inputs, every operation rounded once and none contracted:
 *     u = (K00 * X + K01 * Y) / Z + K02        v = (K11 * Y) / Z + K12
 * then each coordinate is snapped to a 1/256-pixel lattice: rint(u * 256), rint(v * 256), ties to even, as 64-bit integers.
 * Dropped faces (documented behaviour, counted nowhere; there is no clipping): a face with any vertex at Z <= z_near (compared in fp64) is
 * dropped whole; so is a face with a snapped coordinate of magnitude above 2^30, a face of zero integer (doubled) area A = (x1 - x0)
 * (y2 - y0) - (y1 - y0)(x2 - x0), and a face with a NaN or an infinity in one of its vertices -- that face and nothing else.
 * Coverage: both windings count (no back-face culling); a face with A < 0 has its corners 1 and 2 exchanged, so A > 0 below.  The centre
 * c = (256 x + 128, 256 y + 128) of pixel (x, y) is tested in exact 64-bit integer edge functions of the snapped corners,
 *     E0 = (x2 - x1)(cy - y1) - (y2 - y1)(cx - x1),  E1 = (x0 - x2)(cy - y2) - (y0 - y2)(cx - x2),  E2 = (x1 - x0)(cy - y0) - (y1 - y0)(cx - x0)
 * (E0 + E1 + E2 = A).  Top-left fill rule, y downwards: the centre is covered when every E_i > 0, or E_i == 0 on an edge (dx, dy) with
 * dy < 0 (a left edge) or dy == 0 and dx > 0 (a top edge).  A centre on an edge shared by two faces of a planar patch belongs to exactly
 * one of them, a centre on a shared vertex to exactly one face of the fan.
 * Depth at a covered centre is perspective-correct, in fp64: w_i = E_i / A (both integers converted to fp64 first),
 *     1 / z = (w0 / z0 + w1 / z1) + w2 / z2,      z = 1 / that sum, rounded to fp32 once on store.
 * Front = the covering face of smallest fp64 z, back = the one of largest; among equal fp64 values the smaller face index wins in both.
 * Bit-reproducible from run to run and independent of the batch composition and the launch geometry: one lane owns a pixel from the first
 * face to the last, faces are visited in ascending index, there are no atomics and nothing depends on the order of the workgroups. */
typedef struct {
    const int* faces; const int* face_offset; const int* vert_count;
    int M;
} vpho_mesh_table;
VPHO_API long long vpho_mesh_raster_bytes(int n, int face_stride);
VPHO_API int vpho_mesh_raster_f32(const vpho_mesh_table* t, const float* verts, int Vmax, const int* mesh_id, const double* K, int n, int H, int W,
                         int face_stride, double z_near, float* depth_front, float* depth_back, int* face_front, int* face_back,
                         void* workspace, void* stream);
/* vpho_render_overlay_u8: composites up to two rasterised layers (hand, object; either may be NULL = absent) over image [n][3][H][W] fp32,
 * the network's normalised input -> out [n][H][W][3] uint8.  A layer = the depth_front / face_front maps of vpho_mesh_raster_f32 with the
 * verts, mesh_id and table (faces, face_offset, M) they were made from, a colour on the 0 .. 255 scale and an opacity in [0, 1].
 * mean_host / std_host: 3 floats each, HOST arrays.  Per pixel, in fp64:
 *     background_c = (image_c * std_c + mean_c) * 255;
 *     the nearer of the two front layers wins (their fp32 depths compared), the hand wins an exact tie;
 *     n = cross(v1 - v0, v2 - v0) of the winning face's camera-space corners, d = K^-1 (x + 0.5, y + 0.5, 1) for the upper-triangular K:
 *         dy = ((y + 0.5) - K12) / K11,  dx = (((x + 0.5) - K02) - K01 * dy) / K00,  dz = 1;
 *     shade = ambient + (1 - ambient) * (|n . d| / (sqrt(n . n) * sqrt(d . d))), sums as (a + b) + c; a zero normal gets the ambient term only;
 *     out_c = (opacity * shade) * colour_c + (1 - opacity) * background_c, clamped to [0, 255], rounded half to even (a NaN gives 0).
 * Where neither layer covers the pixel, out_c = background_c clamped and rounded the same way.  n == 0: success without a launch. */
typedef struct {
    const float* depth_front; const int* face_front; const float* verts; const int* mesh_id;
    const int* faces; const int* face_offset;
    int Vmax, M;
    float red, green, blue, opacity;
} vpho_render_layer;
VPHO_API int vpho_render_overlay_u8(const float* image, const float* mean_host, const float* std_host, const double* K, const vpho_render_layer* hand,
                           const vpho_render_layer* obj, float ambient, int n, int H, int W, unsigned char* out, void* stream);

/* ---- physics branch of the training step (lib/model/VPHO.py:170-172,205-212 under loss.backward()) -------------------------------
 * backward of vpho_cross_tokens_f32 (cross_module.py:125-133: .view(bs,32,-1) of the projected maps, cat, + positional code):
 * dtok [bs][65][512] -> d_proj_hand / d_proj_obj [bs][8][8][256] NHWC (NULL for the stream the reference detaches, VPHO.py:170-171)
 * and d_grav_emb [bs][512] (may be NULL) */
VPHO_API int vpho_cross_tokens_bwd_f32(const float* dtok, int bs, float* d_proj_hand, float* d_proj_obj, float* d_grav_emb, void* stream);
/* backward of vpho_add_layernorm_f32 (norm1 / norm2 of nn.TransformerEncoderLayer, post-norm): dy -> dx = d(x + r) and dy_xhat =
 * dy * normalised input per element (d gamma = its column sums, d beta = the column sums of dy) */
VPHO_API int vpho_layernorm_bwd_f32(const float* x, const float* r, const float* gamma, const float* dy, long long rows, int E, float eps,
                           float* dx, float* dy_xhat, void* stream);
/* backward of vpho_mha_dropout_f32 (nn.MultiheadAttention inside the encoder layer, sequence axis = batch, quirk Q3):
 * qkv [S*B][3E], d_out [S*B][E], drop_mask as in the forward (NULL = none) -> dqkv [S*B][3E]; S <= 64 (one launch, tables in LDS) */
VPHO_API int vpho_mha_bwd_f32(const float* qkv, const float* d_out, int S, int B, int E, int nhead, const float* drop_mask, float* dqkv, void* stream);
/* the same for S <= 1024 (a per-rank training batch above 64 images): above 64 positions three launches over a workspace of
 * vpho_mha_bwd_workspace_bytes (two S x S tables per (b, head); 0 for S <= 64, which runs the one-launch kernel; -1 = bad argument) */
VPHO_API long long vpho_mha_bwd_workspace_bytes(int S, int B, int nhead);
VPHO_API int vpho_mha_bwd_ws_f32(const float* qkv, const float* d_out, int S, int B, int E, int nhead, const float* drop_mask, float* dqkv,
                        void* workspace, void* stream);
/* HeadPhysics tail + losses + gradient (physics.py:546-557 get_local_force with the double soft-max of :659-664, :362-371
 * from_local_to_global on the GROUND-TRUTH vertices, :456-500 get_loss; weights as VPHO.py:214-219): scale_raw [bs*32] (fc_scale
 * output), logits [bs*32][8] (fc_weight before its Softmax), com [bs*32][3] (fc_CoM output); frame [bs][32][3][3] / point
 * [bs][32][3] from vpho_anchor_frames_f32 of gt_hand_vert_flip; gt_force_local [bs][32][3]; gravity, gt_com [bs][3] in the flipped
 * frame; weights5 (HOST array) = weight_{force,gravity,torque,supervised,CoM}_loss.  Outputs: force_local [bs*32][3], the weighted
 * losses losses5 (device, fp64, same order) and d(total)/d(scale_raw | logits | com).  partial_ws: bs*5 doubles. */
VPHO_API int vpho_physics_loss_f32(const float* scale_raw, const float* logits, const float* com, const float* anchor, float friction,
                          const float* frame, const float* point, const float* gt_force_local, const float* gravity,
                          const float* gt_com, const unsigned char* is_grasped, const float* weights5, int bs,
                          float* force_local, float* d_scale, float* d_logits, float* d_com, double* losses5, double* partial_ws,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
