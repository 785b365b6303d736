/*
 * smoe_hip.h -- C ABI of libsmoe_hip.so: the MI355X (gfx950) implementation of the
 * per-block Steered-Mixture-of-Experts fit / reconstruction hot path.
 *
 * The reference (roljon/Steered-Mixture-of-Experts, /root/reference) has no FFI or
 * plugin interface: its only seam is Python -> tf.Session.run().  Each entry point
 * below replaces one group of session.run() calls of the reference; the reference
 * lines are cited per function.  A maintainer binds these with ctypes (see
 * INTEGRATION.md); the signatures carry plain pointers and sizes only.
 *
 * Semantics: every image block is an independent model ("one Smoe instance per
 * block"): own [0,1]^d pixel domain, own K kernels, own Adam state.  B blocks are
 * processed by one launch.
 *
 * Memory: every array argument is CALLER-OWNED DEVICE memory (hipMalloc'd or a
 * torch tensor's data_ptr()) on the handle's device unless it says "host".  The
 * library allocates only a small workspace inside the handle.  Calls are
 * asynchronous on the hipStream_t passed as `stream` (NULL = default stream).
 *
 * Errors: every call returns SMOE_OK (0) or a negative smoe_status; no exceptions,
 * no aborts.  smoe_last_error() returns a thread-local message for the last failure.
 *
 * Threading: a handle is bound to one device and is not thread-safe; use one handle
 * per device (one process per GPU).  No global state besides the error string.
 */
#ifndef SMOE_HIP_H
#define SMOE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMOE_ABI_VERSION 2
#define SMOE_MAX_DIM 3
#define SMOE_MAX_CHANNELS 3

typedef enum smoe_status {
    SMOE_OK = 0,
    SMOE_ERR_INVALID = -1,      /* bad argument / shape                                  */
    SMOE_ERR_UNSUPPORTED = -2,  /* (dim, channels, kernels) combination not instantiated */
    SMOE_ERR_HIP = -3,          /* a HIP runtime call failed                             */
    SMOE_ERR_NO_DEVICE = -4     /* no usable gfx950 device                               */
} smoe_status;

/* Hyper-parameters of the model + optimiser.  Defaults a caller should use are the
 * smoe_test.py CLI defaults (smoe_test.py:262-352) with kernel adding off. */
typedef struct smoe_config {
    int32_t abi_version;        /* = SMOE_ABI_VERSION                                                    */
    int32_t device;             /* HIP device ordinal                                                    */
    int32_t dim;                /* d: 2 (image) or 3 (video)              smoe.py:227                   */
    int32_t block_shape[SMOE_MAX_DIM]; /* pixels per block per axis (y, x[, t]); unused axes = 1  smoe.py:231-245 */
    int32_t channels;           /* C                                      smoe.py:542                   */
    int32_t kernels;            /* K kernels per block                    smoe.py:2156-2161             */
    int32_t precision;          /* bits of the pixel lattice (8)          utils.py:126-131              */
    float   margin;             /* epsilon = margin / 2^precision         smoe.py:931                   */
    int32_t use_determinant;    /* Gaussian normalisation by prod diag(A) smoe.py:809-815               */
    int32_t use_yuv;            /* 6/8,1/8,1/8 channel loss weights       smoe.py:933-935               */
    int32_t train_pis;          /* trainable flags                        smoe.py:389-396               */
    int32_t train_gammas;
    int32_t train_musx;
    float   lr_expert;          /* optimizer1 {nu_e, gamma_e, musX}       smoe_test.py:84, smoe.py:1102 */
    float   lr_pis;             /* optimizer2 {pis}                       smoe_test.py:85, smoe.py:1103 */
    float   lr_steer;           /* optimizer3 {A_diagonal, A_corr}        smoe_test.py:86, smoe.py:1104 */
    float   beta1, beta2, adam_eps;   /* tf.train.AdamOptimizer defaults .9/.999/1e-8                    */
    float   grad_clip;          /* clip(grad, +-v) if > 0                 smoe.py:1152-1153             */
    float   pis_l1;             /* pis_l1 * sum(pis) / start_pis          smoe.py:1027                  */
    float   u_l1;               /* u_l1 * sum(diag A)                     smoe.py:1044                  */
    int32_t start_pis;          /* normaliser K0 of the l1 term           smoe.py:264,1025              */
    int32_t only_y_gamma;       /* slopes only for channel 0 (gamma_mask) smoe.py:725-729               */
    int32_t ssim_opt;           /* loss_pixel = 1 - SSIM instead of the margin loss (2-d / 3-d blocks, every axis >= 5
                                   pixels): custom_ssim on SYMMETRIC-padded blocks, 11x11(x11) Gaussian, channel
                                   weights 6/8,1/8,1/8 (yuv) or the mean; loss_w is ignored as in the reference
                                   smoe.py:929,980-1011, ops/image_ops_impl.py:77-233                     */
    /* Fake-quantised variables inside the graph (smoe.py:474-538): forward, gradients and update_kernel_list see
     * tf.quantization.fake_quant_with_min_max_{args,vars} of the variables; Adam keeps updating the raw ones.
     * 5-tuples in the reference's order A, musX, nu_e, pis, gamma_e (smoe_test.py:302-309). */
    int32_t quantization_mode;  /* 0/1: nothing in the graph; 2: fixed ranges lower/upper_bounds; 3: min/max over the
                                   block's kernels with qpis > 0 (A_diagonal and nu_e as x - min)   smoe.py:482-530.
                                   Mode 3 assumes A_corr is zero on and above its diagonal (as the reference keeps it) */
    int32_t quantize_pis;       /* pis through [lower_bounds[3], upper_bounds[3]] (implied by mode >= 2). NOTE: the
                                   reference CLI passes True by default (smoe_test.py:304, smoe.py:474)           */
    int32_t bit_depths[5];
    float   lower_bounds[5];
    float   upper_bounds[5];
    int32_t train_inverse_cov;  /* A symmetric (diag + A_corr + A_corr^T), maha = r^T A r; the determinant factor keeps
                                   prod(diag A).  Reference CONSTRUCTOR default True, CLI default False
                                   (smoe.py:41,734-735,791-793; smoe_test.py:342)                               */
    int32_t radial_as;          /* one steering value per kernel (A = a I): the caller keeps A_diagonal [B,K,d,d] with equal
                                   diagonal entries (and equal Adam slots); their gradient is the trace of dL/dA, A_corr
                                   is not trained                                    smoe.py:349-365,429-434,714-719 */
    int32_t kernel_count_as_norm_l1; /* pis_l1 * sum(pis) / count(qpis > 0) instead of / start_pis     smoe.py:1022-1027 */
} smoe_config;

/* Parameter set in the reference's get_params() layout (smoe.py:1795-1800) with a
 * leading block axis B, fp32, C-contiguous:
 *   pis[B,K]  musX[B,K,d]  A_diagonal[B,K,d,d]  A_corr[B,K,d,d]  gamma_e[B,K,d,C]  nu_e[B,K,C]
 * Only the diagonal of A_diagonal and the strict lower triangle of A_corr are read or
 * written (smoe.py:732-733); the other entries are carried untouched. */
typedef struct smoe_params {
    float* pis;
    float* musX;
    float* A_diagonal;
    float* A_corr;
    float* gamma_e;
    float* nu_e;
} smoe_params;

/* TF1 Adam slots (m, v per variable, same layout as smoe_params) and the running
 * beta powers, which TF keeps per optimizer and multiplies after every apply. */
typedef struct smoe_adam_state {
    smoe_params m;
    smoe_params v;
    float   beta1_power;        /* host, in/out; initialise to beta1 */
    float   beta2_power;        /* host, in/out; initialise to beta2 */
    int64_t step;               /* host, in/out; number of applied steps */
} smoe_adam_state;

typedef struct smoe_context* smoe_handle;

/* Create / destroy a handle.  Replaces Smoe.__init__ -> init_model graph construction
 * (smoe.py:229,313,331-1064): builds the per-block pixel domain linspace(0,1,size) per
 * axis (gen_domain, smoe.py:2395-2426) on the device. */
int smoe_create(smoe_handle* out, const smoe_config* cfg);
int smoe_destroy(smoe_handle h);

/* 1 if the (dim, channels, kernels) combination has a compiled kernel (csrc/smoe_variants.def). */
int smoe_is_supported(int32_t dim, int32_t channels, int32_t kernels);

/* The smallest instantiated kernel count >= `kernels` for (dim, channels), or -1.  The reference accepts any kernel
 * grid (generate_kernel_grid, smoe.py:2146-2163); a caller whose count is not instantiated pads every block to this
 * count with kernels of prior 0: `bool_mask = kernel_list & pis > 0` (smoe.py:480,738) takes them out of the graph,
 * their gradients are 0 and ApplyAdam leaves a variable with zero slots and zero gradient where it is. */
int smoe_padded_kernels(int32_t dim, int32_t channels, int32_t kernels);
/* The same over the triples built with EVERY graph variant (ssim_opt, quantization_mode 2 / 3; the lines marked FULL in
 * csrc/smoe_variants.def): what a caller pads to when its graph needs one of those kernels. */
int smoe_padded_kernels_full(int32_t dim, int32_t channels, int32_t kernels);

/* Copy the device-resident per-pixel coordinates [d][N] (fp32) to a HOST buffer. */
int smoe_get_coords(smoe_handle h, float* host_out);

/* Evaluation pass.  Replaces run_batched(train=False, update_reconstruction=True)
 * (smoe.py:1606-1793; fetches at 1646-1648,1686-1697): for every block computes the
 * gate, the reconstruction and the loss with the block's current active-kernel mask,
 * then replaces the mask by the kernels that have influence (smoe.py:829-836,1763-1766).
 *   target  [B,C,N] fp32 in [0,1] (channel-planar per block)      loss_w [B,N] or NULL (smoe.py:550)
 *   recon   [B,C,N] or NULL  (quantised reconstruction, smoe.py:857,899)
 *   argmax  [B,N] uint8 or NULL (smoe.py:833 mapped to kernel ids as at smoe.py:1706-1716)
 *   gate_w  [B,K,N] or NULL  (masked gate, smoe.py:837, zero rows for pruned kernels)
 *   loss    [B]  loss_op (smoe.py:1051)      sse [B]  sum of squared error (mse_op = sse/(N*C)*(2^p)^2, smoe.py:1053)
 *   active  [B] uint32 bit k = kernel k in kernel_list, in/out; update_active=0 leaves it unchanged */
int smoe_forward(smoe_handle h, int32_t num_blocks, const float* target, const float* loss_w,
                 const smoe_params* p, float* recon, uint8_t* argmax, float* gate_w,
                 float* loss, float* sse, uint32_t* active, int32_t update_active, void* stream);

/* n_iters training iterations.  Replaces the loop body of Smoe.train (smoe.py:1521-1529):
 * run_batched(train=True) = zero accumulators (1613), forward + tf.gradients (1702,1148),
 * kernel-list prune (1763-1766), one ApplyAdam per group (1788,1173-1193), and the
 * per-iteration divergence test (1565-1570, per block).
 *   p, s      in/out           loss_last/sse_last [B]: values of the LAST train pass (may be NULL).  A frozen block makes
 *                              no pass: its entries keep the values of its last one, and are left as the caller passed
 *                              them if it was frozen when the call started -- pass the same (initialised) arrays to
 *                              consecutive calls and they read the same however the iterations are split over calls.
 *                              The entries of such a block are NOT written: arrays passed uninitialised hold garbage there
 *   active    [B] in/out       diverged [B] uint32 in/out (non-zero = block frozen), may be NULL
 *   loss0     [B] iteration-0 loss for the blow-up test, or NULL (NaN test only)
 * A tensor that is not trained -- its group's learning rate is 0, train_pis / train_musx / train_gammas is 0 for it, the
 * slopes only_y_gamma masks, A_corr under radial_as -- is dropped from the optimizer as in the reference (smoe.py:1112-1117):
 * the variable AND both of its Adam slots leave the call bit for bit as they entered it, in every block and on every tiling
 * (the slots do not decay towards 0 as they would under a dense step with a zero gradient).  The beta powers and `step`
 * advance all the same.  smoe_shared_apply / smoe_shared_fit treat an untrained tensor the same way. */
int smoe_fit(smoe_handle h, int32_t num_blocks, const float* target, const float* loss_w,
             smoe_params* p, smoe_adam_state* s, int32_t n_iters,
             float* loss_last, float* sse_last, uint32_t* active, uint32_t* diverged,
             const float* loss0, void* stream);

/* Kernel re-admission.  Replaces update_kernel_list (smoe.py:2287-2365) for a per-block
 * [0,1]^d domain: active |= (pis > 0) & any_probe(maha < 800), probes = {min,max,mid}^d. */
int smoe_update_kernel_list(smoe_handle h, int32_t num_blocks, const smoe_params* p,
                            uint32_t* active, void* stream);

/* Best snapshot.  Replaces checkpoint_best_op (smoe.py:861-896, trigger 1574-1576), per
 * block: where loss[b] < best_loss[b] copy p -> best and loss -> best_loss. */
int smoe_checkpoint_best(smoe_handle h, int32_t num_blocks, const float* loss, float* best_loss,
                         const smoe_params* p, smoe_params* best, void* stream);

/* Block -> scalars.  Replaces the host accumulation of smoe.py:1758-1759,1761:
 * out_dev[0] = sum_b loss[b]*N, out_dev[1] = sum_b sse[b], out_dev[2] = sum_b popcount(active[b]).
 * out_dev: 3 doubles in DEVICE memory (ready for an RCCL all-reduce by the host layer). */
int smoe_reduce_scalars(smoe_handle h, int32_t num_blocks, const float* loss, const float* sse,
                        const uint32_t* active, double* out_dev, void* stream);

/* Decoder: evaluate fitted block models on a separable sampling grid and store the samples at their place in the
 * stitched image.  Unlike smoe_forward it needs no target and computes no loss; the sample grid is free (zoom, a finer
 * pitch, frames between the fitted ones), and the output is the interleaved row-major image [E_0, E_1(, E_2), C] that
 * get_reconstruction() returns, not block planes.
 *   first_block, num_blocks  the blocks [first_block, first_block + num_blocks) of the image-wide block grid, row-major
 *                            over grid[] with the last axis innermost (sliding_window order); a rank that holds these
 *                            blocks renders its share into a full-size buffer
 *   p, active                leading axis = num_blocks (the shard), as in smoe_forward; active [num_blocks] is only read,
 *                            NULL = every kernel on the list.  Kernels count when listed and pis > 0; the parameters go
 *                            through the handle's fake quantisation (quantize_pis, quantization_mode 2 / 3 with the
 *                            centre grid of smoe_set_center_grid, indexed like p) exactly as in smoe_forward
 *   axis_coords[l], samples[l]  per axis a DEVICE table of samples[l] fp32 coordinates in block units (the unit in which
 *                            the training lattice is linspace(0, 1, block_shape[l])), the same for all blocks; sample
 *                            (j_0, j_1[, j_2]) of a block is evaluated at (axis_coords[0][j_0], axis_coords[1][j_1], ...).
 *                            Values outside [0, 1] are legal
 *   grid[l], extent[l]       blocks per axis and extent E_l in samples of the WHOLE image, 1 <= E_l <= grid[l]*samples[l];
 *                            block (g_0, g_1[, g_2]) owns positions g_l*samples[l] + j_l, positions >= E_l are not written
 *                            (the crop of a ragged image).  Offsets into the image are 64-bit
 *   image, image_format      SMOE_IMAGE_F32: the lattice values smoe_forward writes into recon (bit-identical on the
 *                            training lattice for the same handle state and num_blocks / smoe_set_total_blocks);
 *                            SMOE_IMAGE_U8: the lattice indices k of k / (2^precision - 1) (precision <= 8)
 *   argmax                   [E_0, E_1(, E_2)] uint8 or NULL: first maximum among the kernels with influence on the
 *                            sample; 255 where no kernel has influence (smoe_forward replaces such pixels by a block-wide
 *                            choice made on the training lattice; a render grid has none, so the 255 stays)
 * Entries [dim .. 2] of the arrays are ignored.  Only positions owned by the rendered blocks are written.  Stores are
 * 16-byte wide when image / argmax are 16-byte aligned. */
#define SMOE_IMAGE_F32 0
#define SMOE_IMAGE_U8 1
int smoe_render(smoe_handle h, int32_t first_block, int32_t num_blocks, const smoe_params* p, const uint32_t* active,
                const float* const axis_coords[3], const int32_t samples[3], const int32_t grid[3],
                const int64_t extent[3], void* image, int32_t image_format, uint8_t* argmax, void* stream);

/* Seam-free decoder: smoe_render, with the models of neighbouring blocks cross-faded in a band around every block border.
 * Every block is fitted alone, so the stitched function jumps at the borders; a fitted block is a continuous function and
 * legal outside [0, 1], so near a border the neighbour is evaluated at the same image position too and the two (2^dim at a
 * corner) are mixed with a partition-of-unity window that is 1/2 : 1/2 on the seam.  Arguments as smoe_render, except:
 *   p, active                cover ALL prod(grid) blocks of the image, indexed by the image-wide block index (row-major over
 *                            grid[]): the neighbours of the rendered range are read.  So does the centre grid of
 *                            smoe_set_center_grid when the handle has one.  Only positions owned by
 *                            [first_block, first_block + num_blocks) are written
 *   blend[l]                 half-width of the band on axis l in SOURCE pixels, finite, 0 <= blend[l] <= block_shape[l] / 2;
 *                            0 (or block_shape[l] == 1): no blending on that axis.  All zero: smoe_render's kernel runs
 * Per axis, with n = block_shape[l], u the sample's coordinate, b = blend[l] / (n - 1), the seams of the own block at
 * s0 = -0.5 / (n - 1) and s1 = 1 + 0.5 / (n - 1): the block at g + 1 gets w_hi = clamp(0.5 * (1 + (u - s1) / b), 0, 1), the block
 * at g - 1 gets w_lo = clamp(0.5 * (1 + (s0 - u) / b), 0, 1), a block outside the image 0, the own block 1 - w_lo - w_hi.  The
 * weight W of a block is the product over the axes.  Every block with W > 0 is evaluated at its own coordinate of the
 * sample (fp32: u - n / (n - 1) seen from g + 1, u + n / (n - 1) from g - 1) exactly as smoe_render evaluates a block; blocks
 * in which no kernel has influence on the sample are dropped (an extrapolated model often loses all its kernels to the
 * threshold); the sample is sum W clip(y, 0, 1) / sum W over the rest, 0 if none is left, put on the lattice once
 * (floor(v (2^precision - 1) + 1/2)).  Samples whose neighbour weights are all 0 are bit-identical to smoe_render's.
 *   argmax                   of the own block only, as smoe_render
 * Limits: with blend not all zero the samples per block may sum to at most 16384 over the axes (smoe_render: 32768), and
 * the workgroup's tables, block records and staging must fit 160 KB of LDS like smoe_render's; beyond that the call returns
 * SMOE_ERR_UNSUPPORTED.  The upper clamp of w_hi / w_lo at 1 only acts on coordinates that leave the own block's footprint by
 * more than the band (blocks.render_axis never produces them); it keeps the own weight from going negative there. */
int smoe_render_blend(smoe_handle h, int32_t first_block, int32_t num_blocks, const smoe_params* p, const uint32_t* active,
                      const float* const axis_coords[3], const int32_t samples[3], const int32_t grid[3],
                      const int64_t extent[3], const float blend[3], void* image, int32_t image_format, uint8_t* argmax,
                      void* stream);

/* Viewport decode: an axis-aligned window of the image on a "ragged separable grid" that owes nothing to the block grid,
 * into a dense image [E_0, E_1(, E_2), C] that holds the window and nothing else.  Per axis l:
 *   view_first[l], view_blocks[l]   the blocks view_first .. view_first + view_blocks - 1 of the axis form the box of the view
 *   axis_start[l]            HOST array of view_blocks[l] + 1 int32: start[0] = 0, non-decreasing, start[view_blocks[l]] = E_l
 *                            >= 1.  Output indices [start[j], start[j + 1]) lie in block view_first[l] + j; empty runs are legal
 *                            (a thumbnail skips blocks) and cost nothing.  Read during the call only
 *   axis_coords[l]           DEVICE table of E_l fp32 coordinates, each in the block units of the block that owns the sample
 *                            (the unit of smoe_render's tables).  The kernel computes no coordinates
 * Sample (i_0, i_1(, i_2)) is evaluated by the block whose per-axis indices own i_l (image-wide index row-major over grid[])
 * at (coords_0[i_0], ...) exactly as smoe_render evaluates a sample of that block; every position of the image is written.
 *   p, active                cover ALL prod(grid) blocks, indexed by the image-wide block index, as does the centre grid of
 *                            smoe_set_center_grid; only the blocks of the box with a non-empty run on every axis and, with
 *                            blend, their neighbours inside the image are read
 *   blend                    NULL, or per-axis half-widths in source pixels with the checks and the meaning of
 *                            smoe_render_blend (same windows, neighbour coordinates, drop of blocks without influence, single
 *                            rounding).  NULL, all zero, or block_shape[l] == 1 on every blended axis: no blending
 *   image_format, argmax     as smoe_render (argmax: uint8 local kernel id of the own block, 255 = none)
 * The hoisting level is the one smoe_render takes for prod(grid) blocks (the tiling of the whole image), so a view on
 * blocks.render_axis coordinates is bit-identical to the same positions of smoe_render / smoe_render_blend.  Results do not
 * depend on how the launch cuts the view into workgroups.  Offsets into the image are 64-bit; stores are 16 bytes wide where
 * image / argmax are 16-byte aligned, element-wise at ragged heads and tails.
 * Limits: E_l <= 2^31 - 1; a block's run may have any length.  A workgroup takes a tile of the view (at most 256 innermost
 * samples, at most 1024 outer tuples) and stages only the tile's part of the tables and the derived records of the blocks the
 * tile touches.  SMOE_ERR_UNSUPPORTED: the derived records of the smallest tile (one block, with blend 3 per blended axis)
 * pass 48 KB, the tile does not fit 160 KB of LDS, the launch would need 2^31 or more workgroups, or SMOE_IMAGE_U8 with
 * precision > 8.  The call uploads its tiling table into a workspace of the handle on `stream`: calls of one handle must be
 * ordered on one stream (as every entry point that uses the handle's workspaces). */
int smoe_render_view(smoe_handle h, const smoe_params* p, const uint32_t* active, const int32_t grid[3],
                     const int32_t view_first[3], const int32_t view_blocks[3], const int32_t* const axis_start[3],
                     const float* const axis_coords[3], const float blend[3], void* image, int32_t image_format,
                     uint8_t* argmax, void* stream);

/* Point decode: the model's value at num_points arbitrary positions that owe nothing to each other -- a rotated or warped
 * view, a motion-compensated lookup, a profile along a line, a set of probes.
 *   points                   DEVICE [num_points, dim] fp32, source pixels in the image's axis order (y, x[, t]); pixel q covers
 *                            [q, q + 1) (the convention of blocks.view_axis)
 *   grid, length             blocks per axis; the true extent of the image in pixels, 1 <= length[l] <= grid[l] * block_shape[l]
 *   p, active                cover ALL prod(grid) blocks, indexed by the image-wide block index, as does the centre grid of
 *                            smoe_set_center_grid
 *   values                   [num_points, C], SMOE_IMAGE_F32 (lattice values) or SMOE_IMAGE_U8 (lattice indices)
 *   argmax                   [num_points] or NULL: uint8 local kernel id of the own block, 255 = none
 *   block                    [num_points] or NULL: int32 image-wide index of the own block, -1 = outside
 * Per axis l, with n = block_shape[l] and x the point's coordinate, all in IEEE fp32:
 *   outside                  x is NaN, x < 0 or x >= length[l] on ANY axis: values 0 (U8: 0), argmax 255, block -1, nothing
 *                            else is computed for the point
 *   block                    the integer g with g n <= x < (g + 1) n exactly: floorf(x / n), corrected by +-1 against the
 *                            products g n and (g + 1) n, which are exact in fp32 -- ownership does not depend on how the
 *                            division rounds
 *   block-unit coordinate    t = x - g n (exact), u = (t - 0.5f) / (float)(n - 1): one rounding in the subtraction, a
 *                            correctly rounded division; u = 0 for n == 1.  On a pixel centre q + 0.5 this is entry q of
 *                            smoe_render's training lattice linspace(0, 1, n), bit for bit
 * The own block (image-wide index row-major over grid[]) is evaluated at (u_0, ...) exactly as smoe_render evaluates a sample of
 * that block for prod(grid) blocks: the same active rule, fake quantisation, centre grid and hoisting level.  With blend (NULL,
 * or per-axis half-widths with the checks and the meaning of smoe_render_blend) the sample is cross-faded with the neighbouring
 * blocks exactly as smoe_render_blend / smoe_render_view do it: the window from u, neighbour coordinates u -+ n / (n - 1),
 * weight 0 for neighbours outside the block grid, blocks without influence dropped, neighbours evaluated without hoisting, one
 * rounding onto the lattice.  argmax is the own block's.  The result for a point depends on its coordinates and the model
 * only: not on num_points, its place in the list, the other points or how the launch is cut.  So the pixel centres of the
 * image as points are bit-identical to smoe_render / smoe_render_blend on the training lattice.
 * A workgroup takes 1024 consecutive points; where the blocks between the per-axis minimum and maximum of their block indices
 * (with blend: widened by one) fit the record budget -- 12 KB of derived records, at most prod(grid) -- it derives them once
 * into LDS, otherwise every lane derives its point's block from global memory; both give the same bits.  Environment
 * SMOE_SAMPLE_RECORDS=n (tuning / test hook) caps the records a workgroup stages; 0: never stage.  Offsets are 64-bit;
 * stores are 16 bytes wide where values / argmax / block are 16-byte aligned, element-wise at ragged heads and tails.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: a null handle, p, grid, length, or
 * (num_points > 0) points / values; grid[l] < 1; length[l] outside 1 .. grid[l] * block_shape[l]; an unknown image_format;
 * num_points < 0; blend as in smoe_render_blend.  SMOE_ERR_UNSUPPORTED: grid[l] * block_shape[l] > 2^24 (block origins must
 * be exact in fp32), SMOE_IMAGE_U8 with precision > 8, 2^31 or more workgroups. */
int smoe_sample(smoe_handle h, const smoe_params* p, const uint32_t* active, const int32_t grid[3],
                const int32_t length[3], const float* points, int64_t num_points, const float blend[3],
                void* values, int32_t image_format, uint8_t* argmax, int32_t* block, void* stream);

/* Point derivative: the exact spatial derivative of the model at num_points arbitrary positions -- what an edge map, a
 * structure tensor, a temporal slope dv/dt, a sub-pixel refinement or a Gauss-Newton alignment needs.  Differences of
 * smoe_sample sit on the 8-bit lattice; this is the closed form.
 *   points, grid, length, p, active, blend     smoe_sample's: the same outside rule, own block g and block-unit coordinate u,
 *                            the same active rule, fake quantisation and centre grid
 *   jac                      [num_points, dim, C] fp32: jac[i, l, c] = dV_c / dx_l per SOURCE PIXEL
 *   values                   [num_points, C] fp32 or NULL: V, the value BEFORE the lattice (not smoe_sample's lattice value)
 *   block                    [num_points] or NULL: int32 image-wide index of the own block, -1 = outside
 * One block b at block-unit position u, over its evaluated kernels k (listed, pis > 0):
 *   gate                     g_k = coef_k exp(-m_k / 2), S = sum_k g_k, w_k = g_k / max(S, 1e-11), M_k = [w_k > tau] (strict)
 *   experts and value        e_kc = nu_kc + sum_l Gamma_klc u_l, y_c = sum_k M_k w_k e_kc, v_c = clip(y_c, 0, nudged_max)
 *   log-gate slope           s_k = d log g_k / du = -A_k z_k with z_k = A_k^T (u - mu_k); train_inverse_cov: s_k = -A_k r_k with
 *                            the symmetric A_k and r_k = u - mu_k
 *   normaliser               sbar = sum_j w_j s_j over all evaluated kernels j when S > 1e-11; 0 on the floor
 *   derivative               dy_c / du_l = sum_k M_k w_k ((s_kl - sbar_l) e_kc + Gamma_klc): the mask is piecewise constant
 *   clip                     dv_c / du_l = dy_c / du_l where clip(y_c) == y_c, else 0 (the fit's straight-through test)
 *   lattice                  ignored: the derivative of the value before floor(v (2^p - 1) + 1/2)
 * Blend (windows, neighbour coordinates u -+ n / (n - 1), weight 0 outside the grid, blocks without influence dropped: all
 * smoe_render_blend's): d|w_l| / du_l = +0.5 / b_l for the high neighbour where its ratio 0.5 (1 + (u - s1) / b) lies strictly
 * inside (0, 1), -0.5 / b_l for the low neighbour where its ratio 0.5 (1 + (s0 - u) / b) does, 0 where the ratio is clamped or
 * the neighbour is outside the grid; W_b is the product over the axes of |w_l| or 1 - |w_l| and dW_b follows by the product
 * rule.  Over the blocks kept, V = sum W_b v_b / sum W_b and dV = (sum (dW_b v_b + W_b dv_b) - V sum dW_b) / sum W_b; a
 * neighbour's dv_b / du needs no chain factor (its coordinate is u plus a constant); no block left: V = 0, dV = 0.
 * Units: jac[i, l, c] = dV_c / du_l / (n_l - 1); 0 on an axis with n_l == 1.  Outside points: jac 0, values 0, block -1.  A
 * point owes nothing to the other points, its place in the list or how the launch is cut.
 * A workgroup takes 512 consecutive points; records are staged as in smoe_sample (SMOE_SAMPLE_RECORDS applies).  Offsets are
 * 64-bit; stores are 16 bytes wide where jac / values / block are 16-byte aligned, element-wise at ragged heads and tails.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: a null handle, p, grid, length, or
 * (num_points > 0) points / jac; grid[l] < 1; length[l] outside 1 .. grid[l] * block_shape[l]; num_points < 0; blend as in
 * smoe_render_blend.  SMOE_ERR_UNSUPPORTED: grid[l] * block_shape[l] > 2^24, 2^31 or more workgroups, more than 160 KB of LDS. */
int smoe_sample_grad(smoe_handle h, const smoe_params* p, const uint32_t* active, const int32_t grid[3],
                     const int32_t length[3], const float* points, int64_t num_points, const float blend[3],
                     float* jac, float* values, int32_t* block, void* stream);

/* Anti-aliased point decode: per output sample the mean of the model over a small regular grid of taps inside the sample's
 * footprint in the source image -- a thumbnail with fewer samples than pixels, a zoomed-out warp, a stabilised video view.
 * smoe_sample takes one position per sample, so a decode coarser than the source aliases; this one integrates over the cell.
 *   points, grid, length, p, active, blend     smoe_sample's; a point is the CENTRE of an output cell
 *   footprint                HOST [dim, dim] fp32, row-major, source pixels: column m is the edge vector of an output cell along
 *                            view axis m (an affine view x = M i + t: footprint = M).  One footprint serves all points of a call
 *   taps                     HOST [dim] int32, 1 <= taps[m] <= 16, prod(taps) <= 64: the taps along view axis m
 *   values                   [num_points, C] or NULL, SMOE_IMAGE_F32 (lattice values) or SMOE_IMAGE_U8 (lattice indices): the mean
 *                            put on the lattice by the rounding smoe_sample applies to its own results, floor(v (2^p - 1) + 1/2)
 *   mean                     [num_points, C] fp32 or NULL: the mean before the lattice
 *   count                    [num_points] uint8 or NULL: the taps inside the image
 *   block                    [num_points] or NULL: int32 image-wide index of the own block of the centre, -1 = centre outside (a
 *                            centre outside with taps inside still gets their mean)
 * Per point x and tap multi-index j (0 <= j_m < taps[m]), all in IEEE fp32:
 *   tap offset               o_m = (float)(2 j_m + 1 - taps[m]) / (float)(2 taps[m]): an exact integer numerator, one correctly
 *                            rounded division
 *   tap position             t_l = x_l, then for m = 0 .. dim-1: t_l = t_l + (F[l][m] * o_m), product and sum rounded separately
 *                            (never fused), so numpy float32 gives the position bit for bit (blocks.area_taps).  With
 *                            taps[m] == 1 the offset is 0 and the tap is the point itself
 *   tap value                the tap is resolved exactly as a point of smoe_sample_grad -- the same outside rule against length,
 *                            own block g and block-unit coordinate u, with blend the same cross-fade -- and its value is that
 *                            call's `values` V (before the lattice), bit for bit
 *   mean                     acc_c = 0, cnt = 0; over the taps in row-major order of j (last axis fastest) an inside tap adds
 *                            acc_c = acc_c + V_c (one fp32 add) and cnt += 1; mean_c = acc_c / (float)cnt, correctly rounded;
 *                            cnt == 0 gives 0.  Taps outside the image are left out, not counted as black: an edge cell of a
 *                            thumbnail stays as bright as its inside
 * No argmax: an average has no single kernel.  The result for a point depends on its coordinates, footprint, taps and the
 * model only: not on num_points, its place in the list, the other points, staging or how the launch is cut.
 * Limits: one footprint per call (an affine view; smoe_sample_area_each takes one per point); at most 64 taps (an 8 x 8 box: a 1/8 thumbnail; 4 x 4 x 4: video);
 * per-block models only -- the counterpart for the whole-image models of smoe_shared_sample is smoe_shared_sample_area.
 * A workgroup takes 256 consecutive points and bounds the blocks of all their taps: the centres' box widened per axis by the
 * footprint's half extent 0.5 sum_m |F[l][m]| plus one block (with blend: one more); records are staged as in smoe_sample where
 * that box fits the budget (SMOE_SAMPLE_RECORDS applies), and both paths give the same bits.  Offsets are 64-bit; stores are 16
 * bytes wide where values / mean / count / block are 16-byte aligned, element-wise at ragged heads and tails.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: smoe_sample's cases (values excepted),
 * a null footprint / taps, a non-finite footprint entry, taps[m] outside 1 .. 16, prod(taps) > 64, (num_points > 0) values and
 * mean both NULL.  SMOE_ERR_UNSUPPORTED: grid[l] * block_shape[l] > 2^24, SMOE_IMAGE_U8 values with precision > 8, 2^31 or more
 * workgroups, more than 160 KB of LDS. */
int smoe_sample_area(smoe_handle h, const smoe_params* p, const uint32_t* active, const int32_t grid[3],
                     const int32_t length[3], const float* points, int64_t num_points, const float* footprint,
                     const int32_t* taps, const float blend[3], void* values, int32_t image_format, float* mean,
                     uint8_t* count, int32_t* block, void* stream);

/* smoe_sample_area with a footprint and tap counts of its own for every point: a view whose magnification varies across the
 * output -- a perspective view (a homography), a lens-distortion or stabilisation map, a fisheye or polar unwrapping, any dense
 * lookup map.  One fused kernel; nothing is materialised per tap.
 *   points, grid, length, p, active, blend, values, image_format, mean, count, block     smoe_sample_area's, with its outside
 *                            rule, its lattice, "a centre outside with taps inside still gets their mean", block = the centre's
 *                            own block, and no argmax
 *   footprints               DEVICE [num_points, dim, dim] fp32, row-major per point, source pixels; any 4-byte address
 *   taps                     DEVICE [num_points, dim] uint8; any address
 * For point i with F = footprints[i], n = taps[i] and tap multi-index j (0 <= j_m < n_m) the arithmetic is smoe_sample_area's
 * statement word for word, in IEEE fp32: o_m = (float)(2 j_m + 1 - n_m) / (float)(2 n_m); t_l = x_l, then for m = 0 .. dim-1
 * t_l = t_l + (F[l][m] * o_m), product and sum rounded separately (blocks.area_taps_each gives the positions bit for bit); taps
 * walked in row-major order of j; an inside tap adds acc_c = acc_c + V_c and cnt += 1; mean_c = acc_c / (float)cnt.  The result
 * for point i is therefore bit for bit the result of smoe_sample_area called with that one point, that footprint and those taps.
 * VOID points: a point is void if any taps[i][m] is outside 1 .. 16, if prod(taps[i]) > 64, or if any entry of footprints[i] is
 * not finite.  A void point gives values 0, mean 0 and count 0; its block is still the centre's own block; it never affects
 * another point.  The host cannot check device arrays, so this is a defined result and there is no error code for it; whatever
 * bytes the arrays hold, the kernel indexes inside its tables and no point takes more than 64 taps.
 * A workgroup takes 256 consecutive points.  The box of blocks it stages bounds every point's taps by the point's own half
 * extents 0.5 sum_m |F[l][m]| (computed in the kernel, not rounded up exactly: a tap whose block falls outside the box is
 * derived directly and gives the same bits, so the box is a performance device only); void points add nothing to it; one point
 * with a huge footprint -- |F| reaches thousands of pixels near a horizon -- sends its workgroup onto the unstaged path, with
 * the same bits (SMOE_SAMPLE_RECORDS applies).  Lanes run their own trip counts; points are never sorted or re-binned.
 * footprints and taps are loaded 16 / 4 bytes wide where their base is aligned so, element-wise otherwise: the same bits.
 * Limits: the equal-weight box filter, at most 16 taps per axis and 64 per point, per-block models only (the counterpart for
 * whole-image models is smoe_shared_sample_area_each).
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: smoe_sample_area's cases (its host
 * footprint / taps checks excepted), plus (num_points > 0) a null footprints or taps.  SMOE_ERR_UNSUPPORTED: as
 * smoe_sample_area. */
int smoe_sample_area_each(smoe_handle h, const smoe_params* p, const uint32_t* active, const int32_t grid[3],
                          const int32_t length[3], const float* points, int64_t num_points, const float* footprints,
                          const uint8_t* taps, const float blend[3], void* values, int32_t image_format, float* mean,
                          uint8_t* count, int32_t* block, void* stream);

/* Name of the kernel variant smoe_fit would launch for num_blocks (diagnostics / profiles). */
const char* smoe_fit_variant(smoe_handle h, int32_t num_blocks);

/* Name of the kernel the LAST smoe_fit call of this handle launched ("" before the first launch): the variant the call
 * chose with ITS arguments -- smoe_fit_variant asks without loss weights, and with them the LDS a block needs grows, so
 * the duo / team rules and the LDS-fit fallback can settle on another kernel -- followed by the tiling suffix
 * (_duo64w2, _team16wN, _pair = one block on both wavefronts of the 64-lane kernel), the graph instantiation
 * (+ssim, +quant, +ic) and the loss-weight marks (+lw: loss_w was passed; +sample: and taken as a pixel sub-sample).
 * Diagnostics / tests: lets a caller assert which kernel a result came from. */
const char* smoe_last_fit_variant(smoe_handle h);

/* Resident wavefronts per CU the runtime grants smoe_fit's kernel for num_blocks (diagnostics). */
int smoe_fit_occupancy(smoe_handle h, int32_t num_blocks);

/* use_diff_center (smoe.py:390-394,746-747: the trained variable is the OFFSET from the kernel grid, the graph reads
 * fake_quant(offset) + grid).  The engines keep grid + offset in musX; with quantization_mode 2 / 3 they need the grid to
 * quantise the offsets: caller-owned device array [num_blocks, K, d] laid out like musX and indexed like the musX of every
 * later smoe_forward / smoe_fit / smoe_update_kernel_list call; it must stay alive until cleared with NULL or the handle
 * is destroyed.  Without quantization_mode 2 / 3 it is not read. */
int smoe_set_center_grid(smoe_handle h, const float* grid);

/* Force the lanes-per-block tiling (16, 32, 64; 0 = automatic).  128 = the 64-lane kernels with ONE block on both
 * wavefronts of a workgroup in smoe_fit (other graphs and the evaluation run the plain 64-lane kernel).  216 / 416 / 816 =
 * the team tiling of smoe_fit with 2 / 4 / 8 wavefronts per workgroup: four blocks per workgroup on the 16-lane layout, the
 * wavefronts split the pixel rows (csrc/smoe_team.hip.h; the automatic choice for small batches of the plain margin-loss
 * graph; other graphs and the evaluation choose as with 0).  264 = the duo tiling of smoe_fit: one block on two symmetric
 * wavefronts with a single joint reduction and the slot owners' state in registers (csrc/smoe_duo.hip.h).  Tuning / test hook. */
int smoe_set_tiling(smoe_handle h, int32_t lanes_per_block);

/* Partition invariance.  The reference walks ALL blocks of an image in one host loop (smoe.py:1643-1702): a block's
 * result does not depend on how many other blocks the pass holds.  Here the lanes-per-block tiling -- and with it the
 * order in which a block's per-pixel gradient terms are summed -- is chosen from the number of blocks, so that a shard
 * of an image (one of R ranks, smoe_fit called with num_blocks = B / R) would round differently from the whole image.
 * total_blocks > 0: every later call of this handle chooses its kernels as if it held total_blocks blocks (the block
 * count of the WHOLE job the calls are shards of), whatever num_blocks it is given: per-block results are then
 * bit-identical for every split of the job into calls / ranks.  0 (the default) = choose from each call's num_blocks. */
int smoe_set_total_blocks(smoe_handle h, int64_t total_blocks);

/* Pixel sub-sampling (run_batched(train=True, sampling_percentage < 100), smoe.py:1664-1667): the reference feeds a random
 * subset of a block's pixels.  Here the caller passes the subset as loss weights (N / n for the drawn pixels, 0 for the
 * others: the same loss and gradients, `mean` over the n drawn pixels).  on != 0 tells the following smoe_fit calls that
 * their loss_w is such a sample: pixels with weight 0 are "not fed", i.e. they take no part in the influence test that
 * prunes the kernel list either (smoe.py:829,1763-1766).  With on == 0 (default) weight-0 pixels are loss-mask pixels,
 * which the reference does feed (smoe.py:1674-1677) and which therefore do vote. */
int smoe_set_sampling(smoe_handle h, int32_t on);

/* ---------------------------------------------------------------------------------------------
 * Shared-kernel image mode: the reference's whole-image fit.  ONE global set of K
 * kernels over the [0,1]^d image domain; the image is cut into batches (sliding_window,
 * smoe.py:18-35); every batch evaluates the kernels of its kernel list (smoe.py:738-753); the
 * gradients of all batches of a pass are accumulated (smoe.py:1148-1150) and one ApplyAdam step
 * follows (smoe.py:1788).  overlap_of_batches > 0 adds the halo: the window's extra pixels only take
 * part in the kernel-list influence test (their loss is cropped, smoe.py:909-923); window pixels outside
 * the image carry all-zero coordinates (np.pad of the joint domain, smoe.py:21,28).
 *   target [NB,C,Nb] (batch-planar, as the block layout)   params: get_params() layout, leading K
 *   lists  [NB, KW] uint32 bitmaps, KW = smoe_shared_list_words(h) = ceil(K/32)
 * For multi-GPU the host layer shards the BATCHES: every call takes the range
 * [first_batch, first_batch + num_batches) and launch-local buffers; between
 * smoe_shared_accumulate and smoe_shared_apply it all-reduces the buffer returned by
 * smoe_shared_grad_buffer (K*P+K doubles) over the ranks (RCCL sum).
 * Decoding: smoe_shared_forward reconstructs the training lattice as batch planes; smoe_shared_render evaluates the same
 * model on any separable sampling grid straight into the interleaved image. */
typedef struct smoe_shared_config {
    int32_t abi_version, device, dim;
    int32_t image_shape[SMOE_MAX_DIM];  /* pixels per axis (y, x[, t]), a multiple of batch_shape (smoe.py:239-241) */
    int32_t batch_shape[SMOE_MAX_DIM];
    int32_t channels, kernels, precision;
    float   margin;
    int32_t use_determinant, use_yuv, train_pis, train_gammas, train_musx;
    float   lr_expert, lr_pis, lr_steer, beta1, beta2, adam_eps, grad_clip, pis_l1, u_l1;
    int32_t start_pis;
    int32_t only_y_gamma;
    int32_t overlap;                    /* overlap_of_batches (smoe.py:244), pixels per side */
    int32_t quantization_mode;          /* as smoe_config; mode 3 ranges are IMAGE-wide min / max  smoe.py:474-530 */
    int32_t quantize_pis;
    int32_t bit_depths[5];
    float   lower_bounds[5];
    float   upper_bounds[5];
    int32_t ssim_opt;                   /* loss_pixel = 1 - SSIM of every batch (2-d, >= 5 pixels per axis)  smoe.py:980-1011 */
    int32_t train_inverse_cov;          /* as smoe_config                                       smoe.py:734-735,791-793 */
    int32_t radial_as;                  /* as smoe_config: A_diagonal [K,d,d] with equal diagonals        smoe.py:714-719 */
    int32_t kernel_count_as_norm_l1;    /* pis_l1 / count(qpis > 0) over the image instead of / start_pis  smoe.py:1022-1027 */
} smoe_shared_config;

typedef struct smoe_shared_context* smoe_shared_handle;

int smoe_shared_create(smoe_shared_handle* out, const smoe_shared_config* cfg);
int smoe_shared_destroy(smoe_shared_handle h);
/* Per-pixel loss weights of the whole image (the graph's loss_weights placeholder fed from Smoe.loss_mask,
 * smoe.py:550,932,1674-1677): caller-owned device array [num_batches][Nb] in batch order, indexed with the GLOBAL
 * batch index by every later forward / accumulate / fit call; it must stay alive until cleared with NULL or the
 * handle is destroyed.  Ignored with ssim_opt, as in the reference. */
int smoe_shared_set_loss_weights(smoe_shared_handle h, const float* loss_w);
/* use_diff_center in the shared-kernel mode: the kernel-grid centres [K, d] (see smoe_set_center_grid). */
int smoe_shared_set_center_grid(smoe_shared_handle h, const float* grid);
int smoe_shared_num_batches(smoe_shared_handle h);
int smoe_shared_list_words(smoe_shared_handle h);

/* run_batched(train=False, update_reconstruction=True) (smoe.py:1606-1793).  recon [nb,C,Nb],
 * argmax [nb,Nb] int32 (global kernel ids), loss/sse [nb]; any output may be NULL. */
int smoe_shared_forward(smoe_shared_handle h, int32_t first_batch, int32_t num_batches, const float* target,
                        const smoe_params* p, float* recon, int32_t* argmax, float* loss, float* sse,
                        uint32_t* lists, int32_t update_lists, void* stream);

/* Decoder of the shared-kernel mode: evaluate the ONE global kernel set on a separable sampling grid and store the samples
 * at their place in the interleaved row-major image [E_0, E_1(, E_2), C] -- the counterpart of smoe_render for whole-image
 * models.  No target, no loss, the lists are only read, overlap plays no part.  The sample grid is free (zoom, a finer
 * pitch, frames between the fitted ones) and a batch may have any number of samples (smoe_shared_forward holds a batch in
 * registers: at most 1024 / 2048 pixels).
 *   first_batch, num_batches the batches [first_batch, first_batch + num_batches) of the handle's batch grid (row-major,
 *                            last axis innermost: sliding_window order); a rank renders its batches into a full-size buffer
 *   p                        the global kernels, as in smoe_shared_forward.  A kernel counts when it is listed and its
 *                            (fake-quantised) prior is > 0; the parameters go through the handle's fake quantisation
 *                            (quantize_pis, quantization_mode 2, mode 3 with the IMAGE-wide ranges of THIS call's parameters,
 *                            the centre grid of smoe_shared_set_center_grid) exactly as in smoe_shared_forward
 *   lists                    launch-local [num_batches, KW] bitmaps (row 0 = batch first_batch), only read; NULL = every
 *                            kernel.  A sample is evaluated with the list of the batch that owns its position
 *   axis_coords[l], samples[l]  samples[l] = samples per BATCH on axis l; the image has E_l = grid_l * samples[l] samples
 *                            (grid_l = image_shape[l] / batch_shape[l]) and axis_coords[l] is a DEVICE table of E_l fp32
 *                            coordinates in image units (the unit in which the training lattice is
 *                            linspace(0, 1, image_shape[l])).  Position j_l belongs to batch index j_l / samples[l] on that
 *                            axis.  Values outside [0, 1] are legal.  Offsets into the image are 64-bit
 *   image, image_format      SMOE_IMAGE_F32: the lattice values smoe_shared_forward writes into recon -- bit-identical to
 *                            it on the training lattice (samples = batch_shape, axis_coords[l] = linspace(0, 1,
 *                            image_shape[l]) in fp32) for the same handle state, parameters and lists;
 *                            SMOE_IMAGE_U8: the lattice indices (precision <= 8)
 *   argmax                   [E_0, E_1(, E_2)] int32 or NULL: GLOBAL kernel id of the first maximum among the kernels with
 *                            influence on the sample, -1 where none has (smoe_shared_forward replaces such pixels by a
 *                            batch-wide choice made on the training lattice; a render grid has none, so the -1 stays)
 * Entries [dim .. 2] of the arrays are ignored.  Only positions owned by the rendered batches are written.  Stores are
 * 16-byte wide when image / argmax are 16-byte aligned.  The result does not depend on how the launch spreads a batch
 * over workgroups (few batches are split; environment SMOE_SHARED_RENDER_SPLIT=n forces n workgroups per batch). */
int smoe_shared_render(smoe_shared_handle h, int32_t first_batch, int32_t num_batches, const smoe_params* p,
                       const uint32_t* lists, const float* const axis_coords[3], const int32_t samples[3],
                       void* image, int32_t image_format, int32_t* argmax, void* stream);

/* Point decoder of the shared-kernel mode: the whole-image model at num_points arbitrary positions, into the dense
 * [num_points, C] -- the counterpart of smoe_sample: a rotated or stabilised view, a profile, a few thousand probes.
 *   p                        the global kernels; fake quantisation (quantize_pis, mode 2, mode 3 with the IMAGE-wide ranges of
 *                            THIS call's parameters) and the centre grid exactly as in smoe_shared_render
 *   lists                    [num_batches, KW] bitmaps of ALL batches of the handle, indexed by the global batch id, only
 *                            read; NULL = every kernel, for every point
 *   points                   DEVICE [num_points, dim] fp32 positions in source pixels, image axis order; pixel q covers
 *                            [q, q + 1)
 *   values                   [num_points, C], SMOE_IMAGE_F32 (lattice values) or SMOE_IMAGE_U8 (lattice indices)
 *   argmax                   [num_points] int32 or NULL: GLOBAL kernel id of the first maximum among the kernels with
 *                            influence on the point, -1 where none has, or outside
 * Per axis l, with nb = batch_shape[l], S = image_shape[l] and x the point's coordinate, all in IEEE fp32:
 *   outside                  x is NaN, x < 0 or x >= S on ANY axis: values 0 (U8: 0), argmax -1, nothing else is computed
 *   owning batch             the integer g with g nb <= x < (g + 1) nb exactly: floorf(x / nb), corrected by +-1 against the
 *                            products g nb and (g + 1) nb, which are exact in fp32 -- ownership does not depend on how the
 *                            division rounds.  A point on a batch boundary g nb belongs to batch g
 *   image-unit coordinate    u = (x - 0.5f) / (float)(S - 1): one rounded subtraction, a correctly rounded division; u = 0
 *                            for S == 1.  On a pixel centre q + 0.5 this is entry q of the training lattice
 *                            linspace(0, 1, S), bit for bit
 * The point is evaluated at (u_0, ...) with the list of its batch exactly as smoe_shared_render evaluates a sample of that
 * batch: the same compacted list (listed and fake-quantised prior > 0, ascending ids), records, sweeps and lattice stage.  Its
 * result depends on its coordinates, the model and its batch's list only -- not on num_points, its place in the list, the
 * other points or how the launch is cut.  So the pixel centres as points are bit-identical to smoe_shared_render on the
 * training lattice (and to the recon of smoe_shared_forward), the empty list gives 0 / -1.
 * A workgroup takes 1024 consecutive points and walks the distinct batches among them in ascending order, compacting and
 * staging one batch's list at a time (about 7 us per batch and workgroup on the MI355X): a row-major view or warp meets
 * 1024 / (samples per batch on the innermost axis) batches per image row a workgroup covers, scattered probes up to one per
 * point -- correct, and slow.  Offsets are 64-bit; stores are 16 bytes wide where values / argmax are 16-byte aligned,
 * element-wise at ragged heads and tails.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: a null handle, p, or
 * (num_points > 0) points / values; num_points < 0; an unknown image_format.  SMOE_ERR_UNSUPPORTED: SMOE_IMAGE_U8 with
 * precision > 8, image_shape[l] > 2^24 (batch origins must be exact in fp32), 2^31 or more workgroups, more than 160 KB of
 * LDS. */
int smoe_shared_sample(smoe_shared_handle h, const smoe_params* p, const uint32_t* lists,
                       const float* points, int64_t num_points,
                       void* values, int32_t image_format, int32_t* argmax, void* stream);

/* Viewport decoder of the shared-kernel mode: a dense view [E_0, E_1(, E_2), C] of the whole-image model given by per-axis
 * tables -- the counterpart of smoe_render_view: only the view is computed and stored (an 8x detail, a thumbnail, one frame).
 *   p, lists                 as in smoe_shared_sample (lists of ALL batches, global batch id; NULL = every kernel)
 *   extent[l]                E_l >= 1 samples on axis l; the image is row-major over extent
 *   axis_coords[l]           DEVICE table of E_l fp32 coordinates in image units (as in smoe_shared_render)
 *   axis_batch[l]            DEVICE table of E_l int32 batch indices on axis l, 0 <= . < grid_l (a value outside is clamped
 *                            into that range): sample (i_0, i_1, ..) is evaluated with the list of batch
 *                            (axis_batch[0][i_0], axis_batch[1][i_1], ..) of the handle's batch grid (row-major)
 *   image, image_format, argmax   as values / argmax of smoe_shared_sample, [E.., C] and [E..]
 * The kernel computes neither coordinates nor ownership here and nothing is outside; a sample is evaluated exactly as
 * smoe_shared_sample evaluates a point with these coordinates in this batch (one kernel family, the same contract), so a
 * view whose tables are a crop of smoe_shared_render's grid is bit-identical to that crop.  Entries [dim .. 2] of the arrays
 * are ignored.  SMOE_ERR_INVALID names the offending argument: a null handle, p, extent, axis_coords, axis_batch, image or
 * table; extent[l] < 1; an unknown image_format.  SMOE_ERR_UNSUPPORTED as in smoe_shared_sample (no limit on image_shape). */
int smoe_shared_render_view(smoe_shared_handle h, const smoe_params* p, const uint32_t* lists,
                            const int32_t extent[3], const float* const axis_coords[3],
                            const int32_t* const axis_batch[3],
                            void* image, int32_t image_format, int32_t* argmax, void* stream);

/* Exact spatial derivative of the whole-image model at arbitrary points -- the counterpart of smoe_sample_grad for the
 * shared-kernel mode, the one model here that is one continuous function without block seams: an edge map, a structure
 * tensor, dv/dt of a video model, a Gauss-Newton alignment step.  Differences of smoe_shared_sample sit on the 8-bit lattice.
 *   p, lists, points, num_points   as in smoe_shared_sample
 *   jac                      DEVICE [num_points, dim, C] fp32: jac[i, l, c] = dv_c / dx_l per source pixel
 *   values                   DEVICE [num_points, C] fp32 or NULL: v, the value before the lattice
 *   batch                    DEVICE [num_points] int32 or NULL: global id of the owning batch, -1 outside
 * Definition.  Points, the outside rule, the owning batch and the image-unit coordinate u are smoe_shared_sample's
 * (u = (x - 0.5f) / (float)(S - 1), 0 for S == 1).  The evaluated kernels of a point are the compacted list of its batch,
 * exactly as in smoe_shared_sample (listed, fake-quantised prior > 0, ascending ids; lists == NULL: every kernel; the same
 * records, mode-3 image-wide ranges and centre grid).  Over them:
 *   g_k = gate of kernel k at u    S = sum g_k    w_k = g_k * rcp(max(S, 10e-12))    M_k = [w_k > tau]
 *   e_kc = nu_kc + sum_l Gamma_klc u_l            y_c = sum_k M_k w_k e_kc           v_c = med3(y_c, 0, nudged_max)
 * The gate and y are formed by the same statements in the same order as smoe_shared_sample forms them, so
 * floorf(fmaf(v_c, inv_scale, 0.5f)) * scale equals smoe_shared_sample's float image bit for bit.
 *   s_k = d log g_k / du = -A_k z_k, z_k = A_k^T (u - mu_k)     (train_inverse_cov: s_k = -A_k (u - mu_k), A_k symmetric)
 *   sbar = sum_j w_j s_j over ALL evaluated kernels, 0 on the floor of the normaliser (S <= 10e-12)
 *   dy_c / du_l = sum_k M_k w_k ((s_kl - sbar_l) e_kc + Gamma_klc)    (the slopes are centred on sbar before they meet the experts)
 *   dv = dy where the clip did not act (v_c == y_c), else 0
 *   jac[i, l, c] = dv_c / du_l / (S_l - 1) per source pixel, 0 on an axis with S_l == 1
 * Mask, clip and lattice are held piecewise constant.  Outside points give 0 / 0 / -1; an inside point whose batch has an
 * empty list gives 0 / 0 / its batch id.  A point's three outputs depend on its coordinates, the model and its batch's list
 * only: not on num_points, its place in the list, the other points or the cut of the launch.
 * A workgroup takes 512 consecutive points and walks the distinct batches among them as smoe_shared_sample does.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: a null handle or p; with
 * num_points > 0 a null points or jac; num_points < 0.  SMOE_ERR_UNSUPPORTED: image_shape[l] > 2^24, 2^31 or more workgroups,
 * more than 160 KB of LDS. */
int smoe_shared_sample_grad(smoe_shared_handle h, const smoe_params* p, const uint32_t* lists,
                            const float* points, int64_t num_points,
                            float* jac, float* values, int32_t* batch, void* stream);

/* The same derivative on a dense view given by per-axis tables: extent, axis_coords and axis_batch are
 * smoe_shared_render_view's (the batch index clamped, nothing outside), jac [E.., dim, C], values [E.., C] or NULL, batch
 * [E..] or NULL as in smoe_shared_sample_grad.  A sample is evaluated exactly as smoe_shared_sample_grad evaluates a point
 * with these coordinates in this batch.  SMOE_ERR_INVALID names the offending argument: a null handle, p, extent,
 * axis_coords, axis_batch, table or jac; extent[l] < 1.  SMOE_ERR_UNSUPPORTED: 2^31 or more workgroups, more than 160 KB of
 * LDS (no limit on image_shape). */
int smoe_shared_render_view_grad(smoe_shared_handle h, const smoe_params* p, const uint32_t* lists,
                                 const int32_t extent[3], const float* const axis_coords[3],
                                 const int32_t* const axis_batch[3],
                                 float* jac, float* values, int32_t* batch, void* stream);

/* Anti-aliased decode of a whole-image model: per point -- the centre of an output cell -- the mean of the model over a small
 * regular grid of taps inside the cell's footprint, every tap with the kernel list of the batch that owns IT: smoe_sample_area
 * for the shared-kernel mode.  A thumbnail or a zoomed-out warp taken with smoe_shared_sample aliases; this integrates.
 *   p, lists, points, num_points   as in smoe_shared_sample (lists covers ALL batches, NULL = every kernel); a point is the
 *                            centre of an output cell
 *   footprint                HOST [dim, dim] fp32, row-major, source pixels: column m is the edge vector of an output cell along
 *                            view axis m (an affine view x = M i + t: footprint = M).  One footprint serves all points of a call
 *   taps                     HOST [dim] int32, 1 <= taps[m] <= 16, prod(taps) <= 64: the taps along view axis m
 *   values                   DEVICE [num_points, C] or NULL, SMOE_IMAGE_F32 (lattice values) or SMOE_IMAGE_U8 (lattice indices)
 *   mean                     DEVICE [num_points, C] fp32 or NULL: the mean before the lattice
 *   count                    DEVICE [num_points] uint8 or NULL: the taps inside the image
 *   batch                    DEVICE [num_points] int32 or NULL: global id of the batch that owns the CENTRE, -1 = centre outside
 *                            (a centre outside with taps inside still gets their mean)
 * Definition, per point x and tap multi-index j (0 <= j_m < taps[m]), all in IEEE fp32:
 *   tap offset               o_m = (float)(2 j_m + 1 - taps[m]) / (float)(2 taps[m]): an exact integer numerator, one correctly
 *                            rounded division
 *   tap position             t_l = x_l, then for m = 0 .. dim-1: t_l = t_l + (F[l][m] * o_m), product and sum rounded separately
 *                            (never fused): exactly smoe_sample_area's, blocks.area_taps gives the position bit for bit
 *   tap value                the tap is resolved exactly as a point of smoe_shared_sample_grad: the outside rule against
 *                            image_shape, the owning batch, u = (t - 0.5f) / (float)(S - 1) (0 for S == 1), the compacted
 *                            list of THAT batch, the gate sums and the clip as the same statements in the same order; its value
 *                            is that call's `values` V (before the lattice), bit for bit
 *   mean                     acc_c = 0, cnt = 0; over the taps in row-major order of j (last axis fastest) an inside tap adds
 *                            acc_c = acc_c + V_c (one fp32 add) and cnt += 1; mean_c = acc_c / (float)cnt, correctly rounded;
 *                            cnt == 0 gives 0.  Taps outside the image are left out, not counted as black.  The order is
 *                            smoe_sample_area's and does not depend on which batches the taps fall in
 *   values                   the mean put on the lattice by the statement smoe_shared_sample ends with,
 *                            floorf(fmaf(mean, inv_scale, 0.5f)), times scale for SMOE_IMAGE_F32, the index for SMOE_IMAGE_U8:
 *                            with one tap smoe_shared_sample's image bit for bit.  Every V is at most nudged_max, but the
 *                            rounded sum of up to 64 of them over their count may pass nudged_max by a few ulp, so the index is
 *                            clamped to the index of nudged_max (no change wherever the mean is within the clip)
 * No argmax: an average has no single kernel.  A point's result depends only on its coordinates, the footprint, the taps, the
 * model and the lists of the batches its taps lie in: not on num_points, its place in the list, the other points or the cut of
 * the launch.  With T = prod(taps) a workgroup takes 512 / T consecutive points, one tap per work item, and walks the distinct
 * batches among their taps as smoe_shared_sample does; there is no table form (a viewport goes through the point form).
 * Offsets are 64-bit; stores are 16 bytes wide where values / mean / count / batch are 16-byte aligned, element-wise at ragged
 * heads and tails.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: smoe_shared_sample's cases (values
 * excepted: a null handle or p, a bad image_format, num_points < 0, with num_points > 0 a null points), a null footprint / taps,
 * a non-finite footprint entry, taps[m] outside 1 .. 16, prod(taps) > 64, (num_points > 0) values and mean both NULL.
 * SMOE_ERR_UNSUPPORTED: image_shape[l] > 2^24, SMOE_IMAGE_U8 values with precision > 8, 2^31 or more workgroups, more than
 * 160 KB of LDS. */
int smoe_shared_sample_area(smoe_shared_handle h, const smoe_params* p, const uint32_t* lists,
                            const float* points, int64_t num_points,
                            const float* footprint, const int32_t* taps,
                            void* values, int32_t image_format,
                            float* mean, uint8_t* count, int32_t* batch, void* stream);

/* smoe_shared_sample_area with a footprint and tap counts of its own for every point: a perspective view, a lens-distortion or
 * stabilisation map, any dense lookup map of a whole-image model -- smoe_sample_area_each for the shared-kernel mode.  One fused
 * kernel; nothing is materialised per tap.
 *   p, lists, points, num_points, values, image_format, mean, count, batch     smoe_shared_sample_area's, with its outside rule,
 *                            its lattice and the clamp of the index, "a centre outside with taps inside still gets their mean",
 *                            batch = the batch of the centre (-1 outside), and no argmax
 *   footprints               DEVICE [num_points, dim, dim] fp32, row-major per point, source pixels; any 4-byte address
 *   taps                     DEVICE [num_points, dim] uint8; any address
 * The result for point i is bit for bit the result of smoe_shared_sample_area called with that one point, footprints[i] and
 * taps[i].  Written out in IEEE fp32 with F = footprints[i], n = taps[i] and tap multi-index j (0 <= j_m < n_m):
 * o_m = (float)(2 j_m + 1 - n_m) / (float)(2 n_m), one correctly rounded division; t_l = x_l, then for m = 0 .. dim-1
 * t_l = t_l + (F[l][m] * o_m), product and sum rounded separately (blocks.area_taps_each gives the positions bit for bit); each
 * tap is resolved and evaluated exactly as a point of smoe_shared_sample_grad, with the list of the batch the tap lies in; taps
 * are summed in row-major order of j, acc_c = acc_c + V_c and cnt += 1 for inside taps; mean_c = acc_c / (float)cnt, correctly
 * rounded, 0 for cnt == 0.
 * VOID points (smoe_sample_area_each's rule): a point is void if any taps[i][m] is outside 1 .. 16, if prod(taps[i]) > 64, or if
 * any entry of footprints[i] is not finite.  A void point gives values 0, mean 0 and count 0; its batch is still the centre's
 * batch; it never affects another point.  The host cannot check device arrays, so this is a defined result and there is no
 * error code for it; whatever bytes the arrays hold, a point contributes at most 64 work items and the kernel indexes inside
 * its tables.
 * A workgroup takes a fixed run of 64 consecutive points -- the host plans the launch without reading device data -- and works
 * through their taps in rounds of 256 (two axes) or 512 (three axes) work items; each round walks the distinct batches among its items as
 * smoe_shared_sample_area does, and the owner lane of a point sums its taps in order across the rounds.  Neighbouring cells
 * are cheap, scattered ones pay a batch walk per distinct batch and round; a small launch of many-tap points runs its rounds
 * serially inside a workgroup (64 points of 64 taps: 16 or 8 rounds) where smoe_shared_sample_area would use 8 workgroups.  Offsets
 * are 64-bit; stores are 16 bytes wide where values / mean / count / batch are 16-byte aligned.
 * Limits: the equal-weight box filter, at most 16 taps per axis and 64 per point, no table (viewport) form.
 * num_points == 0 is a successful no-op.  SMOE_ERR_INVALID names the offending argument: smoe_shared_sample_area's cases (its
 * host footprint / taps checks excepted), plus (num_points > 0) a null footprints or taps.  SMOE_ERR_UNSUPPORTED:
 * image_shape[l] > 2^24, SMOE_IMAGE_U8 values with precision > 8, 2^31 or more workgroups, more than 160 KB of LDS. */
int smoe_shared_sample_area_each(smoe_shared_handle h, const smoe_params* p, const uint32_t* lists,
                                 const float* points, int64_t num_points,
                                 const float* footprints, const uint8_t* taps,
                                 void* values, int32_t image_format,
                                 float* mean, uint8_t* count, int32_t* batch, void* stream);

/* run_batched(train=True) minus train_op: forward + tf.gradients of the batches, accumulated into
 * the handle's gradient buffer (accum_ops, smoe.py:1150); kernel lists pruned (smoe.py:1763-1766).
 * Summation order: every batch leaves the raw sums of its listed kernels in a row of its own; the buffer is the sum of
 * the rows of ALL batches accumulated since the last step, per kernel in batch order (fp64) -- bit-identical from run to run
 * and for any split of a rank's batches over calls.  (Only if the rows would exceed 4 GB -- num_batches x kernels x ~10..22
 * floats -- the pass falls back to fp64 atomics, whose order is not fixed.) */
int smoe_shared_accumulate(smoe_shared_handle h, int32_t first_batch, int32_t num_batches, const float* target,
                           const smoe_params* p, float* loss, float* sse, uint32_t* lists, void* stream);

/* train_op (smoe.py:1788): one ApplyAdam step per optimizer group on the accumulated gradients; clears
 * the accumulators (zero_op, smoe.py:1613). */
int smoe_shared_apply(smoe_shared_handle h, smoe_params* p, smoe_adam_state* s, void* stream);

/* zero_op alone (smoe.py:1613): drop what the smoe_shared_accumulate calls since the last step have accumulated. */
int smoe_shared_discard(smoe_shared_handle h, void* stream);

/* Device pointer + length (in doubles) of the gradient accumulation buffer. */
int smoe_shared_grad_buffer(smoe_shared_handle h, double** dev_ptr, int64_t* count);

/* n_iters x (accumulate over ALL batches; apply): the single-GPU loop body of Smoe.train.  Two launches per iteration.
 * Environment SMOE_SHARED_ONE_LAUNCH=1: all n_iters iterations in ONE cooperative launch (grid barriers between the pass and
 * the step; bit-identical results; used when every batch fits on the device at once, margin loss, quantization_mode != 3) --
 * measured slower on MI355X, so it is opt-in.  If such a launch had to give up (a grid barrier timed
 * out), the next smoe_shared_fit / smoe_shared_forward call of the handle returns SMOE_ERR_HIP. */
int smoe_shared_fit(smoe_shared_handle h, const float* target, smoe_params* p, smoe_adam_state* s, int32_t n_iters,
                    float* loss_last, float* sse_last, uint32_t* lists, void* stream);

/* update_kernel_list (smoe.py:2287-2365) for the batches of the range. */
int smoe_shared_update_kernel_list(smoe_shared_handle h, int32_t first_batch, int32_t num_batches,
                                   const smoe_params* p, uint32_t* lists, void* stream);

const char* smoe_last_error(void);
int smoe_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SMOE_HIP_H */
