// smoe_device.h -- argument blocks shared by the kernels (smoe_block.hip.h, smoe_kernels.hip, smoe_shared.hip) and the
// C-ABI host layer (smoe_capi.hip).  Internal; the public surface is include/smoe_hip.h.
#ifndef SMOE_DEVICE_H
#define SMOE_DEVICE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "smoe_hip.h"

namespace smoe {

// What the fit kernels start a block's "loss / SSE of the last pass" from: a signalling-NaN pattern that no arithmetic
// produces (results are quieted) and that only selects carry.  A block that is frozen when the launch starts makes no pass,
// still holds the pattern at the write-back and leaves its loss_last / sse_last entries as the caller passed them: what a
// caller reads there does not depend on how the iterations were split over launches.
#define SMOE_NO_PASS_BITS 0x7fa0deadu
#if defined(__FINITE_MATH_ONLY__) && __FINITE_MATH_ONLY__
#error "SMOE_NO_PASS_BITS is a NaN pattern carried in a float: do not build these kernels with -ffinite-math-only / -ffast-math"
#endif
#if defined(__HIPCC__)
__device__ __forceinline__ float no_pass_value() { return __uint_as_float(SMOE_NO_PASS_BITS); }
__device__ __forceinline__ bool made_a_pass(float last) { return __float_as_uint(last) != SMOE_NO_PASS_BITS; }
#endif

// Block-independent constants of the forward / loss maths.
struct KernelConsts {
    float tau;          // 0.5 / 2^p                       smoe.py:825
    float epsm;         // margin / 2^p                    smoe.py:931
    float scale;        // 1 / (2^p - 1)                   fake_quant nudged scale, smoe.py:899
    float inv_scale;    // 1 / scale
    float nudged_max;   // min(1, (2^p - 1) * scale): upper clamp of clip_by_value + fake quant
    float cw[SMOE_MAX_CHANNELS];  // per-channel loss weight / N   smoe.py:933-937
    float n_dis;        // sqrt((2 pi)^d)                  smoe.py:812
    float inv_n_dis;    // 1 / n_dis
    int use_det;        // smoe.py:809
    int train_gammas;   // smoe.py:841
    int only_y_gamma;   // gamma_mask: slopes only for channel 0 (smoe.py:725-729)
    float sw[SMOE_MAX_CHANNELS];  // ssim_opt: SSIM channel weight / window count (smoe.py:1006-1009)
    // fake-quantised parameters inside the graph (smoe.py:474-538).  Group order: 0 A, 1 musX, 2 nu_e, 3 pis, 4 gamma_e
    int qmode;          // 0 none, 2 fixed ranges (lower/upper_bounds), 3 min/max over the model's kernels
    int qpis;           // pis through the fixed range (mode >= 2 or quantize_pis)
    int q_musx;         // mode 3 quantises musX only when it is trained (smoe.py:515)
    float q_nmin[5], q_nmax[5], q_scale[5], q_inv[5];   // nudged fixed ranges (TF Nudge(), fp32)
    float q_levels[5];  // 2^bits - 1
    int inverse_cov;    // train_inverse_cov (smoe.py:734-735,791-793): A symmetric, maha = r^T A r
    int radial;         // radial_as (smoe.py:714-719): the steering diagonal is one value per kernel
    int kcount_norm;    // kernel_count_as_norm_l1: pis l1 term normalised by count(qpis > 0) (smoe.py:1022-1027)
    float pis_l1_raw;   // the un-normalised pis_l1 for that
};

struct FitArgs {
    const float* target;      // [B,C,N]
    const float* loss_w;      // [B,N] or null
    smoe_params p, m, v;
    float* loss_out;          // [B] or null
    float* sse_out;           // [B] or null
    uint32_t* active;         // [B]
    uint32_t* diverged;       // [B] or null
    const float* loss0;       // [B] or null
    const float* coords;      // [D][N]
    int B, N, n_iters;
    float b1p, b2p, beta1, beta2, eps;
    float lr_expert, lr_pis, lr_steer;
    int train_pis, train_musx;
    float clip;
    float reg_pi;             // pis_l1 / start_pis
    float reg_u;              // u_l1
    const float* ssim_T;      // ssim_opt: banded tap tables Tr [bh][11], Tc [bw][11], 3-d blocks: Tt [bt][11] (null otherwise)
    int bh, bw, bt;
    int desc_off;             // float offset of the owner-side gradient descriptors in the dynamic LDS (set by the launcher; 0 = off)
    const float* mus_grid;    // use_diff_center with quantization_mode 2 / 3: kernel-grid centres [B,K,D] (null otherwise)
    int pair;                 // few blocks: one block per 2-wavefront workgroup (64-lane tiling, margin loss; fit_kernel PAIR)
    int lds_floats;           // dynamic LDS of the launch in floats (set by the launcher; read by the SMOE_DEBUG carve-up checks)
    uint32_t* dbg;            // SMOE_DEBUG build: device word that collects failed device-side checks (null otherwise)
    int prio_rotate;          // the launch is ONE round (every wavefront resident at once): rotate the wavefronts' priorities (smoe_block.hip.h)
    int lw_is_sample;         // loss_w is a pixel sub-sample (smoe_set_sampling): weight-0 pixels are not fed, they do not vote in the kernel-list prune
    KernelConsts kc;
};

struct FwdArgs {
    const float* target;
    const float* loss_w;
    smoe_params p;
    float* recon;             // [B,C,N] or null
    uint8_t* argmax;          // [B,N] or null
    float* gate_w;            // [B,K,N] or null
    float* loss;              // [B] or null
    float* sse;               // [B] or null
    uint32_t* active;         // [B]
    const float* coords;
    int B, N, update_active;
    int hoist;                // trailing axes whose coordinate is a lane constant (same rule as smoe_fit)
    const float* mus_grid;    // as in FitArgs
    int regt;                 // evaluation kernel: targets in registers, no staged planes in LDS (set by the launcher)
    float reg_pi, reg_u;
    const float* ssim_T;
    int bh, bw, bt;
    int lds_floats;           // as in FitArgs
    uint32_t* dbg;
    KernelConsts kc;
};

struct ReadmitArgs {
    smoe_params p;
    uint32_t* active;
    const float* probes;      // [D][3] = {min, max, mid} per axis
    int B, K;
    int inverse_cov;          // train_inverse_cov: maha = r^T A r
    const float* mus_grid;    // as in FitArgs
};

struct BestArgs {
    const float* loss;
    float* best_loss;
    smoe_params p, best;
    int B, K, D, C;
};

struct ReduceArgs {
    const float* loss;
    const float* sse;
    const uint32_t* active;
    double* out;
    double* partials;         // [reduce_partials_count()] workspace of the handle
    int B, N;
};

// smoe_render (smoe_render.hip.h): evaluate the blocks [first, first + nb) of an image-wide block grid on a separable sample
// grid and store the samples into the stitched image.  The launcher fills the geometry fields.
struct RenderArgs {
    smoe_params p;            // leading axis = nb (the shard)
    const uint32_t* active;   // [nb] or null = every kernel listed
    const float* ax[SMOE_MAX_DIM];   // per-axis sample coordinates in block units
    int m[SMOE_MAX_DIM];      // samples per block and axis
    int grid[SMOE_MAX_DIM];   // blocks per axis of the whole image
    long long ext[SMOE_MAX_DIM];     // extent of the whole image in samples
    int first, nb;
    void* image;              // [E_0, E_1(, E_2), C] float32 or uint8
    int fmt;                  // SMOE_IMAGE_F32 / SMOE_IMAGE_U8
    uint8_t* argmax;          // [E_0, E_1(, E_2)] or null
    const float* mus_grid;    // as in FitArgs, indexed like p
    int vec_img, vec_arg;     // the plane's base is 16-byte aligned: vector stores
    int NB, CL, RP;           // blocks per workgroup, innermost samples per block and pass, outer sample tuples per step
    int chunks, line0;        // workgroups per grid line, first grid line of the launch
    int off_par, off_stage;   // float offsets of the block images / the staging buffers in the dynamic LDS
    KernelConsts kc;
};

// smoe_render_blend (smoe_render_blend.hip.h): smoe_render with a cross-fade towards the neighbouring blocks around every
// block border.  r.p / r.active / r.mus_grid cover ALL prod(grid) blocks and are indexed by the image-wide block index.
struct RenderBlendArgs {
    RenderArgs r;
    float s0[SMOE_MAX_DIM], s1[SMOE_MAX_DIM];   // the own block's seams in block units: -0.5 / (n - 1), 1 + 0.5 / (n - 1)
    float band[SMOE_MAX_DIM];                   // half-width of the blend band in block units, blend / (n - 1); 0: none on this axis
    float pitch[SMOE_MAX_DIM];                  // one block in block units, n / (n - 1)
    int off_w;                                  // float offset of the neighbour-weight tables in the dynamic LDS (launcher)
};

// smoe_render_view (smoe_render_view.hip.h): a window of the image on a ragged separable sample grid.  r.p / r.active /
// r.mus_grid cover ALL prod(grid) blocks (image-wide block index); r.ax[l]: the E_l coordinates of axis l; r.ext[l] = E_l;
// r.CL / r.RP: columns of a tile / rows per step; r.off_par / r.off_stage: the derived records / the staging buffers.
struct RenderViewArgs {
    RenderArgs r;
    float s0[SMOE_MAX_DIM], s1[SMOE_MAX_DIM], band[SMOE_MAX_DIM], pitch[SMOE_MAX_DIM];   // as in RenderBlendArgs; band 0: no blend on the axis
    const int32_t* tab;       // device table of the launch (ViewPlan::tab); per axis, at these offsets:
    int o_ent_start[SMOE_MAX_DIM];   // [entries + 1] first sample of every non-empty run ("entry"), then E_l
    int o_ent_slot[SMOE_MAX_DIM];    // [entries] the entry's block in the axis' record list
    int o_rec_block[SMOE_MAX_DIM];   // [slots] block index on the axis of every record slot: the entries' blocks, ascending, with a
                                     // blend on the axis also their neighbours inside the image
    int o_tile_s[SMOE_MAX_DIM];      // [tiles + 1] first sample of every tile, then E_l
    int o_tile_e[SMOE_MAX_DIM];      // [tiles][2] the entries [first, end) a tile touches
    int ntiles[SMOE_MAX_DIM];
    int TS[SMOE_MAX_DIM];            // samples of the largest tile on the axis: the size of its LDS tables
    int off_ax[SMOE_MAX_DIM];        // float offset of the axis' tables in the dynamic LDS
};

// the host tables of a view as the caller of smoe_render_view passed them
struct ViewHost {
    const int32_t* start[SMOE_MAX_DIM];
    int32_t first[SMOE_MAX_DIM], blocks[SMOE_MAX_DIM];
};

// what render_view_layout makes for the device next to the geometry fields of RenderViewArgs
struct ViewPlan {
    std::vector<int32_t> tab;
};

// smoe_sample (smoe_sample.hip.h): the model at a list of arbitrary positions.  r.p / r.active / r.mus_grid cover ALL
// prod(grid) blocks (image-wide block index); r.image: the values [N, C]; r.argmax: [N] or null; r.off_par / r.off_stage: the
// staged records / the staging buffers.  The launcher fills rec_cap and the offsets.
struct SampleArgs {
    RenderArgs r;
    float s0[SMOE_MAX_DIM], s1[SMOE_MAX_DIM], band[SMOE_MAX_DIM], pitch[SMOE_MAX_DIM];   // as in RenderBlendArgs; band 0: no blend on the axis
    const float* points;      // [N, D] source pixels
    long long num_points;
    int32_t* block;           // [N] image-wide index of the own block (-1: outside) or null
    int vec_blk;              // block's base is 16-byte aligned: vector stores
    int n[SMOE_MAX_DIM];      // pixels per block and axis
    float length[SMOE_MAX_DIM];      // true extent of the image in pixels
    int rec_cap;              // a workgroup stages the records of its box when the box has at most this many blocks
};

// smoe_sample_grad (smoe_sample_grad.hip.h): the model's spatial derivative at a list of arbitrary positions.  s: the points, the
// blocks and the blend as for smoe_sample (s.r.image / s.r.argmax are not used); s.block: [N] or null.
struct SampleGradArgs {
    SampleArgs s;
    float* jac;               // [N, D, C] dV_c / dx_l per source pixel
    float* values;            // [N, C] the value before the lattice, or null
    int vec_jac, vec_val;     // the plane's base is 16-byte aligned: vector stores
    float du_dx[SMOE_MAX_DIM];       // block units per source pixel, 1 / (n - 1); 0 on an axis of one pixel per block
};

// smoe_sample_area (smoe_sample_area.hip.h): the mean of the model over a regular grid of taps inside the footprint of every
// point.  s: the cell centres, the blocks and the blend as for smoe_sample; s.r.image / s.r.fmt: the lattice values [N, C] or
// null; s.r.argmax is not used; s.block: the centre's own block [N] or null.
constexpr int SAMPLE_AREA_AXIS_TAPS = 16;       // taps per axis, at most
constexpr int SAMPLE_AREA_TAPS = 64;            // taps per point, at most
struct SampleAreaArgs {
    SampleArgs s;
    float F[SMOE_MAX_DIM * SMOE_MAX_DIM];       // the footprint [dim, dim] row-major, source pixels: column m = the cell's edge along view axis m
    int taps[SMOE_MAX_DIM];                     // taps per view axis (1 on the axes past dim)
    int ntaps;                                  // their product
    float half[SMOE_MAX_DIM];                   // half extent of the footprint per source axis, 0.5 sum_m |F[l][m]|, rounded up
    float* mean;              // [N, C] the mean before the lattice, or null
    uint8_t* count;           // [N] taps inside the image, or null
    int vec_mean, vec_cnt;    // the plane's base is 16-byte aligned: vector stores
    int off_tap;              // float offset of the tap table in the dynamic LDS (launcher)
};

// smoe_sample_area_each (smoe_sample_area_each.hip.h): smoe_sample_area with a footprint and tap counts of its own for every
// point.  s, mean, count as in SampleAreaArgs.
struct SampleAreaEachArgs {
    SampleArgs s;
    const float* footprints;  // [N, dim, dim] row-major per point, source pixels
    const uint8_t* taps;      // [N, dim] taps per view axis
    float* mean;              // [N, C] the mean before the lattice, or null
    uint8_t* count;           // [N] taps inside the image, or null
    int vec_mean, vec_cnt;    // the plane's base is 16-byte aligned: vector stores
    int vec_fp, vec_tap;      // footprints' base is 16-byte aligned / taps' base is 4-byte aligned: wide loads
    int off_tab;              // float offset of the offset table o[n][j] in the dynamic LDS (launcher)
    int off_fp, off_tap;      // float offsets of the workgroup's footprints and tap counts in the dynamic LDS (launcher)
};

// What the launcher of a block decoder derives from checked arguments, next to the geometry fields of RenderArgs (and off_w
// of RenderBlendArgs) it fills: a pure host computation (render_layout / render_blend_layout), also run without a device
struct RenderLayout {
    int hl;                   // the hoisting level the launch runs with
    size_t lds_bytes;         // dynamic LDS of a workgroup
    long long workgroups;
};

// The graph a fit or evaluation launch runs; with the tiling (Variant) it names one kernel instantiation
// (resolve_fit / resolve_fwd in smoe_block.hip.h).
struct Graph {
    bool ssim;     // ssim_opt: loss_pixel = 1 - SSIM
    bool quant;    // quantization_mode 2 / 3: every variable fake-quantised
    bool ic;       // train_inverse_cov
    bool pair;     // fit: one block on both wavefronts of a workgroup (plain graph, 64-lane tiling)
    bool outs;     // evaluation: the launch stores recon / gate_w / argmax
};

struct Variant {
    int D, C, K, G, W;
    const char* name;
    bool full;                // built with the SSIM and quantization_mode 2 / 3 kernels (smoe_variants.def)
    hipError_t (*fit)(const FitArgs&, Graph, int hoist_level, hipStream_t);      // hipErrorNotSupported: no kernel for the graph
    hipError_t (*fwd)(const FwdArgs&, Graph, hipStream_t);
    size_t (*lds_bytes)(Graph, int N, bool has_lw, int bh, int bw, int bt);      // (size_t)-1: no kernel for the graph
    int (*fit_waves_per_cu)(int N, bool has_lw, int hoist_level, bool pair);     // of the plain / pair fit kernel
    hipError_t (*readmit_quant)(const ReadmitArgs&, const KernelConsts&, hipStream_t);   // fake-quantised graph
    // team tiling (smoe_team.hip.h; entries of the 16-lane variants only): four blocks per workgroup of nw wavefronts
    hipError_t (*fit_team)(const FitArgs&, int hoist_level, int nw, hipStream_t);
    size_t (*team_lds_bytes)(int N, bool has_lw, int nw);
    int (*team_waves_per_cu)(int N, bool has_lw, int nw);
    // duo tiling (smoe_duo.hip.h; entries of the 64-lane variants only): one block on two symmetric wavefronts
    hipError_t (*fit_duo)(const FitArgs&, int hoist_level, hipStream_t);
    size_t (*duo_lds_bytes)(int N, bool has_lw, int hoist_level);      // (size_t)-1: the triple has too many slots
    int (*duo_waves_per_cu)(int N, bool has_lw, int hoist_level);
    // decoder (smoe_render.hip.h; the same entry on every tiling of a triple): hl = hoisting level, lanes = the tiling's G
    hipError_t (*render)(const RenderArgs&, int hl, int lanes, hipStream_t);
    // seam-free decoder (smoe_render_blend.hip.h), same conventions
    hipError_t (*render_blend)(const RenderBlendArgs&, int hl, int lanes, hipStream_t);
    // the launch geometry of the two decoders alone: what render / render_blend compute before they launch, for the same arguments
    hipError_t (*render_layout)(RenderArgs&, int hl, int lanes, RenderLayout&);
    hipError_t (*render_blend_layout)(RenderBlendArgs&, int hl, int lanes, RenderLayout&);
    // viewport decoder (smoe_render_view.hip.h): the plan of a view (tiling, device table, LDS carve-up: pure host code), and the
    // launch of a planned view whose table is on the device
    hipError_t (*render_view_layout)(RenderViewArgs&, const ViewHost&, ViewPlan&, int hl, RenderLayout&);
    hipError_t (*render_view)(const RenderViewArgs&, const RenderLayout&, hipStream_t);
    // point decoder (smoe_sample.hip.h): the geometry of a call (pure host code; records: the caller's cap on the staged records,
    // < 0 none), and the launch of a planned call
    hipError_t (*sample_layout)(SampleArgs&, int hl, long long records, RenderLayout&);
    hipError_t (*sample)(const SampleArgs&, const RenderLayout&, hipStream_t);
    // point derivative (smoe_sample_grad.hip.h), same conventions
    hipError_t (*sample_grad_layout)(SampleGradArgs&, long long records, RenderLayout&);
    hipError_t (*sample_grad)(const SampleGradArgs&, const RenderLayout&, hipStream_t);
    // area-averaged point decoder (smoe_sample_area.hip.h), same conventions
    hipError_t (*sample_area_layout)(SampleAreaArgs&, long long records, RenderLayout&);
    hipError_t (*sample_area)(const SampleAreaArgs&, const RenderLayout&, hipStream_t);
    // area-averaged point decoder with per-point footprints (smoe_sample_area_each.hip.h), same conventions
    hipError_t (*sample_area_each_layout)(SampleAreaEachArgs&, long long records, RenderLayout&);
    hipError_t (*sample_area_each)(const SampleAreaEachArgs&, const RenderLayout&, hipStream_t);
};

// ---- shared-kernel image mode (smoe_shared.hip) ----------------------------------------------
struct SharedArgs {
    const float* target;      // [nb][C][Nb] of the batches [b0, b0+nb)
    smoe_params p;            // global kernels [K,...]
    const float* axis_coords; // per-axis global coordinate tables, concatenated
    int axis_off[SMOE_MAX_DIM];
    int batch_shape[SMOE_MAX_DIM];
    int grid[SMOE_MAX_DIM];   // batches per axis
    int image_shape[SMOE_MAX_DIM];
    int overlap;              // halo width (pixels per side) used by the influence test only
    uint32_t* lists;          // [nb][KW] kernel-list bitmaps
    int b0, NB, Nb, K, KW;    // NB = batches in this launch
    float* loss;              // [nb] or null
    float* sse;               // [nb] or null
    float* recon;             // [nb][C][Nb] or null
    int32_t* argmax;          // [nb][Nb] or null
    double* racc;             // [K][PK] raw gradient sums (train)
    double* nact;             // [K] number of batches that listed the kernel (train, for the l1 terms)
    int update_lists;
    KernelConsts kc;
    float reg_pi, reg_u;
    const float* loss_w;      // [num_batches][Nb] per-pixel loss weights of the WHOLE image (global batch index) or null
    const float* ssim_T;      // ssim_opt: banded tap tables Tr [bh][11], Tc [bw][11]
    int ssim;                 // 1: loss_pixel = 1 - SSIM of the batch
    int ssim_off;             // float offset of the SSIM planes inside the workgroup's LDS
    const float* qrng;        // image-wide records of shared_ranges_kernel (mode 3 ranges, count of qpis > 0); see SharedRangesArgs
    const float* mus_grid;    // use_diff_center with quantization_mode 2 / 3: kernel-grid centres [K][D] (null otherwise)
    // fixed-order gradient accumulation (train passes): every batch leaves the raw sums of its listed kernels in its own rows
    // part[global batch][kernel][PK] and the set of those kernels in trained[global batch][KW], stamped with the pass number
    // (batch_epoch); SharedGatherArgs sums them per kernel in batch order.  part == null: fp64 atomics into racc / nact.
    float* part;
    uint32_t* trained;
    uint32_t* batch_epoch;
    uint32_t epoch;
};

// smoe_shared_render (smoe_shared_render.hip.h): evaluate the batches [b0, b0 + nb) of the image on a separable sample grid
// with their kernel lists and store the samples into the interleaved image.  The launcher fills tiles / split.
struct SharedRenderArgs {
    smoe_params p;            // global kernels [K,...]
    const uint32_t* lists;    // launch-local [nb][KW] bitmaps (row 0 = batch b0), only read; null = every kernel
    const float* ax[SMOE_MAX_DIM];   // per-axis sample coordinates of the WHOLE image [E_l], image units
    int m[SMOE_MAX_DIM];      // samples per batch and axis
    int grid[SMOE_MAX_DIM];   // batches per axis
    long long ext[SMOE_MAX_DIM];     // E_l = grid_l * m_l
    int b0, nb, K, KW;
    void* image;              // [E_0, E_1(, E_2), C] float32 or uint8
    int fmt;                  // SMOE_IMAGE_F32 / SMOE_IMAGE_U8
    int32_t* argmax;          // [E_0, E_1(, E_2)] global kernel ids, -1 = no kernel has influence; or null
    int vec_img, vec_arg;     // the plane's base is 16-byte aligned: vector stores
    int tiles, split;         // tiles of SR_TILE samples per batch, workgroups per batch
    const float* qrng;        // as in SharedArgs
    const float* mus_grid;    // as in SharedArgs
    KernelConsts kc;
};

// smoe_shared_sample / smoe_shared_render_view (smoe_shared_sample.hip.h): the model at num_points positions, every one with
// the list of the batch that owns it.  Either the list `points` (source pixels; batch and coordinate made by the kernel) or
// the dense row-major view of `ext` with one coordinate table ax[l] and one batch-index table ab[l] per axis.
struct SharedSampleArgs {
    smoe_params p;            // global kernels [K,...]
    const uint32_t* lists;    // [num_batches][KW] bitmaps of ALL batches (global batch id), only read; null = every kernel
    const float* points;      // [N, D] source pixels (list mode)
    long long num_points;     // N, or prod(ext)
    const float* ax[SMOE_MAX_DIM];    // view mode: [ext_l] coordinates in image units
    const int32_t* ab[SMOE_MAX_DIM];  // view mode: [ext_l] batch index on the axis
    int ext[SMOE_MAX_DIM];    // view mode: samples per axis
    int nbs[SMOE_MAX_DIM];    // batch_shape
    int grid[SMOE_MAX_DIM];   // batches per axis
    int shape[SMOE_MAX_DIM];  // image_shape
    int K, KW;
    void* image;              // [N, C] float32 or uint8
    int fmt;                  // SMOE_IMAGE_F32 / SMOE_IMAGE_U8
    int32_t* argmax;          // [N] global kernel ids, -1 = no kernel has influence, or outside; or null
    int vec_img, vec_arg;     // the plane's base is 16-byte aligned: vector stores
    const float* qrng;        // as in SharedArgs
    const float* mus_grid;    // as in SharedArgs
    KernelConsts kc;
};

// smoe_shared_sample_grad / smoe_shared_render_view_grad (smoe_shared_sample_grad.hip.h): the spatial derivative at the points
// of `s` (its image / argmax planes are unused), the value before the lattice and the owning batch.
struct SharedSampleGradArgs {
    SharedSampleArgs s;
    float* jac;               // [N, D, C] dv_c / dx_l per source pixel
    float* values;            // [N, C] the value before the lattice, or null
    int32_t* batch;           // [N] global batch ids, -1 = outside; or null
    int vec_jac, vec_val, vec_bat;    // the plane's base is 16-byte aligned: vector stores
    float du_dx[SMOE_MAX_DIM];        // 1 / (image_shape[l] - 1), 0 for an axis of one pixel
};

// smoe_shared_sample_area (smoe_shared_sample_area.hip.h): the mean of the model over a regular grid of taps inside the
// footprint of every point of `s` (list mode only), every tap with the list of the batch that owns it.  s.image / s.fmt: the
// lattice values [N, C] or null; s.argmax is not used.
struct SharedSampleAreaArgs {
    SharedSampleArgs s;
    float F[SMOE_MAX_DIM * SMOE_MAX_DIM];       // the footprint [dim, dim] row-major, source pixels: column m = the cell's edge along view axis m
    int taps[SMOE_MAX_DIM];                     // taps per view axis (1 on the axes past dim)
    int ntaps;                                  // their product T, 1 .. SAMPLE_AREA_TAPS
    int ppw;                                    // points per workgroup, SSA_TILE / T (launcher)
    float* mean;              // [N, C] the mean before the lattice, or null
    uint8_t* count;           // [N] taps inside the image, or null
    int32_t* batch;           // [N] global id of the batch that owns the centre, -1 = centre outside; or null
    int vec_mean, vec_cnt, vec_bat;   // the plane's base is 16-byte aligned: vector stores
};

// smoe_shared_sample_area_each (smoe_shared_sample_area_each.hip.h): smoe_shared_sample_area with a footprint and tap counts of
// its own for every point of `s` (list mode only).  s, mean, count, batch as in SharedSampleAreaArgs.
struct SharedSampleAreaEachArgs {
    SharedSampleArgs s;
    const float* footprints;  // [N, dim, dim] row-major per point, source pixels; any 4-byte address
    const uint8_t* taps;      // [N, dim] taps per view axis; any address
    float* mean;              // [N, C] the mean before the lattice, or null
    uint8_t* count;           // [N] taps inside the image, or null
    int32_t* batch;           // [N] global id of the batch that owns the centre, -1 = centre outside; or null
    int vec_mean, vec_cnt, vec_bat;   // the plane's base is 16-byte aligned: vector stores
};

// Per-kernel sum over the batches of the current pass, in a fixed order (lane = batch mod 64 ascending, then a butterfly
// over the lanes): racc[k][PK] and nact[k] are OVERWRITTEN -- bit-identical from run to run and for every split of the
// batches of a rank over smoe_shared_accumulate calls.
struct SharedGatherArgs {
    const float* part;
    const uint32_t* trained;
    const uint32_t* batch_epoch;
    uint32_t epoch;
    int NB_total, K, KW, PK;
    double* racc;
    double* nact;
};

struct SharedAdamArgs {
    smoe_params p, m, v;
    double* racc;
    double* nact;
    int K;
    float b1p, b2p, beta1, beta2, eps, clip;
    float lr_expert, lr_pis, lr_steer;
    int train_pis, train_musx, train_gammas, use_det, only_y_gamma;
    float reg_pi, reg_u;
    KernelConsts kc;          // fake quant of the variables (quantize_pis, quantization_mode 2 / 3)
    float* qrng;              // records of shared_ranges_kernel for the CURRENT parameters (mode 3, kernel_count_as_norm_l1)
    const float* mus_grid;    // as in SharedArgs
    SharedGatherArgs gather;  // gather.part != null: the step sums the batches' rows itself (single launch per step, smoe_shared_fit)
};

struct SharedReadmitArgs {
    smoe_params p;
    uint32_t* lists;          // [nb][KW]
    const float* probes;      // [nb][D][3]
    int NB, K, KW;
    KernelConsts kc;
    const float* qrng;
    const float* mus_grid;    // as in SharedArgs
};

// Image-wide quantities of the fake-quantised graph, recomputed from the parameters before every launch that reads them:
// record t = 0..4 (A_diagonal, A_corr, musX, nu_e, gamma_e) = 8 floats {nudged min, nudged max, step, 1/step, offset
// added back, zero-range flag, raw min, raw max} of quantization_mode 3 (min / max over the kernels with qpis > 0,
// smoe.py:497-530); qrng[40] = count(qpis > 0) (kernel_count_as_norm_l1, smoe.py:1012,1022-1027).
static constexpr int SHARED_QRNG_FLOATS = 48;
struct SharedRangesArgs {
    smoe_params p;
    float* qrng;
    int K;
    KernelConsts kc;
    const float* mus_grid;    // as in SharedArgs
};

// smoe_shared_fit as one launch (shared_fit_kernel): the pass and step arguments of the first iteration (the kernel advances the
// pass number and the beta powers itself), the iteration count, and the device words of the grid barrier, zeroed by the host
// before the launch: bar[2] abort, bar[8 .. 11] phase clocks of the diagnostic build, bar[16 + w] arrival flag of workgroup w
// (16 + NB rounded up to a multiple of four words)
struct SharedFitArgs {
    SharedArgs pass;
    SharedAdamArgs adam;
    int n_iters;
    uint32_t* bar;
};

size_t shared_lds_bytes(int D, int C, int K, int KW);
size_t shared_ssim_lds_bytes(int C, int Nb, int bh, int bw, int bt);
bool shared_supported(int D, int C, int Nb);
hipError_t launch_shared_pass(const SharedArgs& a, int D, int C, bool train, hipStream_t st);
hipError_t launch_shared_adam(const SharedAdamArgs& a, int D, int C, hipStream_t st);
hipError_t launch_shared_gather(const SharedGatherArgs& g, hipStream_t st);
// hipErrorCooperativeLaunchTooLarge: the batches do not all fit on the device at once (the caller keeps its two launches per
// iteration); num_cus = compute units of the device
hipError_t launch_shared_fit(const SharedFitArgs& f, int D, int C, int num_cus, hipStream_t st);
hipError_t launch_shared_readmit(const SharedReadmitArgs& a, int D, hipStream_t st);
hipError_t launch_shared_ranges(const SharedRangesArgs& a, int D, int C, hipStream_t st);
// split_hint > 0: workgroups per batch (test / tuning hook); 0: chosen from nb and num_cus.  hipErrorNotSupported: more than
// 2^30 samples per batch
hipError_t launch_shared_render(const SharedRenderArgs& a, int D, int C, int num_cus, int split_hint, hipStream_t st);
// the geometry of a smoe_shared_sample / smoe_shared_render_view call (pure host code; g.hl is unused and 0).
// hipErrorNotSupported: 2^31 or more workgroups, or more than 160 KB of LDS
hipError_t shared_sample_layout(int D, int C, int K, long long num_points, RenderLayout& g);
// the launch of a planned call; grid: the dense view of a.ext / a.ax / a.ab instead of the list a.points
hipError_t launch_shared_sample(const SharedSampleArgs& a, int D, int C, bool grid, const RenderLayout& g, hipStream_t st);
// the same pair for smoe_shared_sample_grad / smoe_shared_render_view_grad
hipError_t shared_sample_grad_layout(int D, int C, int K, long long num_points, RenderLayout& g);
hipError_t launch_shared_sample_grad(const SharedSampleGradArgs& q, int D, int C, bool grid, const RenderLayout& g, hipStream_t st);
// the same pair for smoe_shared_sample_area; T = prod(taps), 1 .. SAMPLE_AREA_TAPS.  The launch fills q.ppw
hipError_t shared_sample_area_layout(int D, int C, int K, int T, long long num_points, RenderLayout& g);
hipError_t launch_shared_sample_area(const SharedSampleAreaArgs& q, int D, int C, const RenderLayout& g, hipStream_t st);
// the same pair for smoe_shared_sample_area_each: a workgroup takes a fixed run of points, so the plan reads no device data
hipError_t shared_sample_area_each_layout(int D, int C, int K, long long num_points, RenderLayout& g);
hipError_t launch_shared_sample_area_each(const SharedSampleAreaEachArgs& q, int D, int C, const RenderLayout& g, hipStream_t st);

const Variant* variants(int* count);
hipError_t launch_readmit(const ReadmitArgs& a, int D, hipStream_t st);
hipError_t launch_best(const BestArgs& a, hipStream_t st);
hipError_t launch_reduce(const ReduceArgs& a, hipStream_t st);
int reduce_partials_count();

}  // namespace smoe
#endif
