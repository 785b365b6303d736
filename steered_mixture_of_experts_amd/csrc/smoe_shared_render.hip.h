// smoe_shared_render.hip.h -- decoder of the shared-kernel image mode: evaluate the ONE global kernel set on a separable
// sampling grid, every sample with the kernel list of the batch whose footprint it lies in, and store the samples at their
// place in the interleaved image [E_0, E_1(, E_2), C] (smoe_shared_render, include/smoe_hip.h).  Included by
// smoe_shared.hip, which owns SL<D, C>, shared_stage_record / shared_gate and the fake-quantisation helpers.
//
// What it runs is step 0 (list compaction), sweeps A and B and the output stage of shared_pass_body through the same
// device functions, in the same order over the compacted list (ascending kernel id): on the training lattice the image is
// bit-identical to the recon of smoe_shared_forward.  No target, no loss, no reduction, no write to the lists, no halo.
//
// Arrangement.  The m_0 x m_1 (x m_2) samples of a batch are numbered row-major (innermost image axis fastest) and cut into
// tiles of SR_TILE = 256 lanes x SR_PXL consecutive numbers; lane `tid` takes the samples n0 + p * 256 + tid of a tile, so
// the 64 lanes of a wavefront sit side by side on the innermost axis.  A workgroup does not hold a batch in registers: it
// walks tiles, so a batch may have any number of samples.  A batch is taken by `split` workgroups (tile t goes to
// workgroup t mod split); each of them compacts and stages the batch's list for itself -- a few hundred floats next to the
// thousands of samples of a tile, and no exchange between workgroups.  A sample is computed by one lane from the same
// staged records whatever the split, so the image does not depend on it.
//
// A list of up to SH_KC kernels (the usual case after a fit has pruned the lists) is staged once per workgroup; a longer
// one is re-staged chunk by chunk for every tile and sweep.
//
// Stores.  A tile is a handful of runs along the innermost image axis (whole rows of the batch, a ragged first / last one).
// The values are turned through LDS and leave as 16-byte non-temporal stores on 16-byte boundaries of the IMAGE when its
// base is aligned, element-wise at the runs' heads / tails (render_store_run of smoe_render.hip.h); uint8 output and
// the kernel-id plane take the same path.
//
// ids: first maximum among the kernels with influence on the sample, -1 where none has.  smoe_shared_forward patches such
// pixels with a batch-wide choice made on the training lattice; a render grid has no such notion, so the -1 STAYS.
#ifndef SMOE_SHARED_RENDER_HIP_H
#define SMOE_SHARED_RENDER_HIP_H

#include "smoe_render.hip.h"

namespace smoe {

constexpr int SR_PXL = 4;                            // samples per lane and tile
constexpr int SR_TILE = SH_THREADS * SR_PXL;

// The runs of tile [n0, n0 + cnt) of a batch, from the staging buffer to the image.  cps: components per sample (C, or 1
// for the id plane); ve = 1 << vs: elements per vector store (1: the plane's base is not 16-byte aligned); org: the batch's
// first sample per axis.
template <int D, bool U8>
__device__ __forceinline__ void shared_render_flush(const SharedRenderArgs& a, const uint32_t* __restrict__ st,
                                                    void* __restrict__ img, const int cps, const int vs, const int n0,
                                                    const int cnt, const int (&org)[D]) {
    const int ve = 1 << vs;
    const int ML = a.m[D - 1];
    const long long EL = a.ext[D - 1];
    const int r0 = n0 / ML, r1 = (n0 + cnt - 1) / ML;
    const int nruns = r1 - r0 + 1;
    const int cpr = (min(ML, cnt) * cps + ve - 1) / ve + 1;      // 16-byte lines a run can touch
    for (int w = threadIdx.x; w < nruns * cpr; w += SH_THREADS) {
        const int run = w / cpr;
        const int ch = w - run * cpr;
        const int o = r0 + run;                                  // outer sample tuple of the run
        const int ja = (run == 0) ? n0 - r0 * ML : 0;
        const int jb = (o == r1) ? n0 + cnt - r1 * ML : ML;
        long long row;
        if (D == 3) {
            const int j0 = o / a.m[1], j1 = o - j0 * a.m[1];
            row = (long long)(org[0] + j0) * a.ext[1] + (org[1] + j1);
        } else {
            row = org[0] + o;
        }
        const long long e0 = (row * EL + org[D - 1] + ja) * cps;
        render_store_run<U8>(st, img, e0, e0 + (long long)(jb - ja) * cps, (o * ML + ja - n0) * cps, vs, ch);
    }
}

template <int D, int C, bool IC>
__global__ void __launch_bounds__(SH_THREADS) shared_render_kernel(SharedRenderArgs a) {
    using L = SL<D, C>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int K = a.K;
    const int b = (int)(blockIdx.x / (unsigned)a.split);             // batch inside this launch (the lists are launch-local)
    const int part = (int)(blockIdx.x - (unsigned)b * (unsigned)a.split);

    // LDS carve-up
    int* s_list = reinterpret_cast<int*>(lds);                       // [K] compacted active kernel ids
    float* s_par = lds + K;                                          // [SH_KC][SP]
    int* s_cnt = reinterpret_cast<int*>(s_par + SH_KC * L::SP);      // [8]
    uint32_t* s_val = reinterpret_cast<uint32_t*>(s_cnt + 8);        // [SR_TILE][C] value bits / lattice indices
    uint32_t* s_arg = s_val + SR_TILE * C;                           // [SR_TILE] kernel ids

    // ---- 0. compact the batch's kernel list: listed & pis > 0, ascending ids (step 0 of shared_pass_body) ----
    const uint32_t* bits = (a.lists != nullptr) ? a.lists + (size_t)b * a.KW : nullptr;
    if (tid == 0) s_cnt[0] = 0;
    __syncthreads();
    for (int kbase = 0; kbase < K; kbase += SH_THREADS) {
        const int k = kbase + tid;
        bool keep = false;
        const int kc_ = (k < K) ? k : K - 1;
        const uint32_t word = (bits != nullptr) ? bits[kc_ >> 5] : 0xffffffffu;
        const float prior = a.p.pis[kc_];
        if (k < K && ((word >> (k & 31)) & 1u)) keep = fqv(prior, a.kc, 3) > 0.0f;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[1 + wave] = __popcll(m);
        __syncthreads();
        int off = s_cnt[0];
        for (int ww = 0; ww < wave; ++ww) off += s_cnt[1 + ww];
        if (keep) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = k;
        __syncthreads();
        if (tid == 0) s_cnt[0] += s_cnt[1] + s_cnt[2] + s_cnt[3] + s_cnt[4];
        __syncthreads();
    }
    const int Kact = s_cnt[0];

    int org[D];                      // the batch's first sample per axis (sliding_window order: last axis fastest)
    {
        int rem = a.b0 + b;
#pragma unroll
        for (int l = D - 1; l >= 0; --l) {
            org[l] = (rem % a.grid[l]) * a.m[l];
            rem /= a.grid[l];
        }
    }
    int M = 1;
#pragma unroll
    for (int l = 0; l < D; ++l) M *= a.m[l];

    int staged_c0 = -1;
    auto stage = [&](int c0, int n) {
        if (c0 == staged_c0) return;
        staged_c0 = c0;
        __syncthreads();
        if (tid < n) shared_stage_record<D, C, IC, false>(a.p, a.kc, a.qrng, a.mus_grid, s_list[c0 + tid], s_par + tid * L::SP);
        __syncthreads();
    };

    const int vs_img = a.vec_img ? ((a.fmt == SMOE_IMAGE_U8) ? 4 : 2) : 0;       // log2 of the elements per 16-byte store
    const int vs_arg = a.vec_arg ? 2 : 0;
    for (int t = part; t < a.tiles; t += a.split) {
        const int n0 = t * SR_TILE;
        const int cnt = min(SR_TILE, M - n0);
        const int np = (cnt + SH_THREADS - 1) / SH_THREADS;          // rounds of the lanes with a sample in this tile

        // ---- 1. this lane's samples: coordinates from the per-axis tables ----
        float x[SR_PXL][D];
        bool pv[SR_PXL];
#pragma unroll
        for (int p = 0; p < SR_PXL; ++p) {
            const int n = n0 + p * SH_THREADS + tid;
            pv[p] = n < M;
            int rem = pv[p] ? n : M - 1;
#pragma unroll
            for (int l = D - 1; l >= 0; --l) {
                const int idx = rem % a.m[l];
                rem /= a.m[l];
                x[p][l] = a.ax[l][org[l] + idx];
            }
        }

        // ---- 2. sweep A: gate normaliser ----
        float S[SR_PXL];
#pragma unroll
        for (int p = 0; p < SR_PXL; ++p) S[p] = 0.0f;
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
#pragma unroll
                for (int p = 0; p < SR_PXL; ++p) {
                    if (p >= np) continue;
                    float z[D];
                    S[p] += shared_gate<D, C, IC>(r, x[p], z);
                }
            }
        }
        float inv[SR_PXL];
#pragma unroll
        for (int p = 0; p < SR_PXL; ++p) inv[p] = frcp(fmaxf(S[p], 10e-12f));

        // ---- 3. sweep B: masked gate, experts, blend, first maximum ----
        float y[SR_PXL][C];
        float best[SR_PXL];
        int arg[SR_PXL];
#pragma unroll
        for (int p = 0; p < SR_PXL; ++p) {
            first_max_init(best[p], arg[p], -1);
#pragma unroll
            for (int c = 0; c < C; ++c) y[p][c] = 0.0f;
        }
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
                const int kid = s_list[c0 + kk];
#pragma unroll
                for (int p = 0; p < SR_PXL; ++p) {
                    if (p >= np) continue;
                    float z[D];
                    const float w = shared_gate<D, C, IC>(r, x[p], z) * inv[p];
                    const float wt = (pv[p] && w > a.kc.tau) ? w : 0.0f;
                    first_max_take(best[p], arg[p], wt, kid);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        float ee = r[L::O_NU + c];
#pragma unroll
                        for (int l = 0; l < D; ++l) ee = fmaf(r[L::O_GA + l * C + c], x[p][l], ee);
                        y[p][c] = fmaf(wt, ee, y[p][c]);
                    }
                }
            }
        }

        // ---- 4. clip + 8-bit lattice (the output stage of shared_pass_body), through LDS to the image ----
#pragma unroll
        for (int p = 0; p < SR_PXL; ++p) {
            const int si = p * SH_THREADS + tid;
            if (si >= cnt) continue;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float yc = __builtin_amdgcn_fmed3f(y[p][c], 0.0f, a.kc.nudged_max);
                const float kq = floorf(fmaf(yc, a.kc.inv_scale, 0.5f));
                s_val[si * C + c] = (a.fmt == SMOE_IMAGE_U8) ? (uint32_t)kq : __float_as_uint(kq * a.kc.scale);
            }
            s_arg[si] = (uint32_t)arg[p];
        }
        __syncthreads();
        if (a.fmt == SMOE_IMAGE_U8) shared_render_flush<D, true>(a, s_val, a.image, C, vs_img, n0, cnt, org);
        else shared_render_flush<D, false>(a, s_val, a.image, C, vs_img, n0, cnt, org);
        if (a.argmax != nullptr) shared_render_flush<D, false>(a, s_arg, a.argmax, 1, vs_arg, n0, cnt, org);
        __syncthreads();                                             // the next tile writes the staging buffer again
    }
}

size_t shared_render_lds_bytes(int D, int C, int K) {
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    return sizeof(float) * (((size_t)K + SH_KC * SP + 8 + (size_t)SR_TILE * (C + 1) + 3) & ~(size_t)3);
}

template <int D, int C>
static hipError_t launch_shared_render_dc(const SharedRenderArgs& a, hipStream_t st) {
    auto kern = (a.kc.inverse_cov != 0) ? shared_render_kernel<D, C, true> : shared_render_kernel<D, C, false>;
    return launch_decoder(kern, (long long)a.nb * a.split, SH_THREADS, shared_render_lds_bytes(D, C, a.K), a, st);
}

// num_cus: compute units of the device; split_hint > 0 forces the workgroups per batch (test / tuning hook), otherwise
// few batches are split until the launch has about four workgroups per compute unit.
hipError_t launch_shared_render(const SharedRenderArgs& a0, int D, int C, int num_cus, int split_hint, hipStream_t st) {
    SharedRenderArgs a = a0;
    long long M = 1;
    for (int l = 0; l < D; ++l) M *= a.m[l];
    if (M > 0x40000000LL) return hipErrorNotSupported;                // sample numbers inside a batch are 32-bit
    a.tiles = (int)((M + SR_TILE - 1) / SR_TILE);
    long long split = (split_hint > 0) ? split_hint : (4LL * (num_cus > 0 ? num_cus : 256) + a.nb - 1) / a.nb;
    if (split > a.tiles) split = a.tiles;
    if (split < 1) split = 1;
    if ((long long)a.nb * split > 0x7fffffffLL) return hipErrorInvalidValue;
    a.split = (int)split;
    if (D == 2 && C == 1) return launch_shared_render_dc<2, 1>(a, st);
    if (D == 2 && C == 3) return launch_shared_render_dc<2, 3>(a, st);
    if (D == 3 && C == 1) return launch_shared_render_dc<3, 1>(a, st);
    if (D == 3 && C == 3) return launch_shared_render_dc<3, 3>(a, st);
    return hipErrorInvalidValue;
}

}  // namespace smoe
#endif
