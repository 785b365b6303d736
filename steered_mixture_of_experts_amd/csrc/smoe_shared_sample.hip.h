// smoe_shared_sample.hip.h -- point and viewport decoder of the shared-kernel image mode: evaluate the ONE global kernel set
// at a list of arbitrary positions (smoe_shared_sample) or on a dense view given by per-axis tables (smoe_shared_render_view),
// every point with the kernel list of the batch that owns it, and store the dense results [N, C] / [E_0, E_1(, E_2), C]
// (include/smoe_hip.h).  Included by smoe_shared.hip after smoe_shared_render.hip.h; it calls that decoder's device functions
// (shared_stage_record, shared_gate, first_max_*, render_store_run) and changes none.
//
// Definition.  GRID = false: a point is D float32 numbers in source pixels, in the image's axis order; pixel q covers
// [q, q + 1).  A point with a NaN, x < 0 or x >= image_shape[l] on any axis is OUTSIDE: values 0, id -1, nothing else is
// computed.  Otherwise per axis its batch is the integer g with g nb <= x < (g + 1) nb (sample_resolve's floor-and-correct
// against the exact products, nb = batch_shape[l]) and its image-unit coordinate is u = (x - 0.5f) / (float)(S - 1), one
// rounded subtraction and one correctly rounded division (0 for S == 1; S = image_shape[l]); blocks.point_blocks states both
// in numpy.  GRID = true: point i is row-major over the extent E; per axis a device table gives the coordinate and the batch
// index of every position, the kernel computes neither and nothing is outside (a batch index outside 0 .. grid_l - 1 is
// clamped: the lists are never read out of bounds).
// A point of batch b is evaluated exactly as shared_render_kernel evaluates a sample of batch b: the list compacted the same
// way (listed and fake-quantised prior > 0, ascending ids), the records of shared_stage_record<D, C, IC, false>, sweep A, the
// reciprocal, sweep B and the clip / lattice stage as the same statements in the same order.  So what a point gives depends on
// its coordinates, the model and its batch's list only: not on N, its place in the list, the other points or the launch.
//
// Arrangement.  A workgroup of 256 lanes takes SS_PPL * 256 consecutive points, lane t the SS_PPL points from t * SS_PPL on
// (as sample_kernel: neighbours in the list are neighbours in a lane and a wavefront).  It resolves its points and then walks
// the DISTINCT batches among them in ascending batch id: every lane offers the smallest batch id of its points above the one
// just done to an LDS atomicMin, the minimum is the next batch -- workgroup-uniform, so every barrier below is reached by all
// 256 lanes.  Per batch the workgroup compacts the batch's list (one lane per list word: one round for K <= 8192), stages it
// (chunks of SH_KC, as the render kernel) and the lanes run sweeps A and B for their points of that batch; a point's
// accumulators live in registers until the end.  A row-major view or warp meets 1024 / (samples per batch on the innermost
// axis) batches per image row it covers; scattered probes meet up to SS_PPL * 256 of them and pay a list compaction and staging
// for each -- about 7 us per batch and workgroup, measured.  The values and ids are turned through LDS and leave
// as one run per plane: 16-byte non-temporal stores where the plane's base is 16-byte aligned, element-wise at the ragged head
// and tail.
#ifndef SMOE_SHARED_SAMPLE_HIP_H
#define SMOE_SHARED_SAMPLE_HIP_H

#include "smoe_sample.hip.h"            // sample_resolve
#include "smoe_shared_render.hip.h"

namespace smoe {

constexpr int SS_PPL = 4;                                // points per lane
constexpr int SS_TILE = SH_THREADS * SS_PPL;             // points per workgroup
constexpr int SS_NONE = 0x7fffffff;                      // "no batch left"

template <int D, int C, bool IC, bool GRID>
__global__ void __launch_bounds__(SH_THREADS) shared_sample_kernel(SharedSampleArgs a) {
    using L = SL<D, C>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int K = a.K;
    const long long p0 = (long long)blockIdx.x * SS_TILE;              // the workgroup's first point
    const long long pe = (a.num_points - p0 < SS_TILE) ? a.num_points : p0 + SS_TILE;

    // LDS carve-up (shared_sample_layout)
    int* s_list = reinterpret_cast<int*>(lds);                       // [K] compacted active kernel ids of the current batch
    float* s_par = lds + K;                                          // [SH_KC][SP]
    int* s_cnt = reinterpret_cast<int*>(s_par + SH_KC * L::SP);      // [8]: 0 list length, 1..4 per wavefront, 5 next batch
    uint32_t* s_val = reinterpret_cast<uint32_t*>(s_cnt + 8);        // [SS_TILE][C] value bits / lattice indices
    uint32_t* s_arg = s_val + SS_TILE * C;                           // [SS_TILE] kernel ids

    // ---- 1. this lane's points: image-unit coordinates and owning batch (-1: outside, or past the end of the list) ----
    float x[SS_PPL][D];
    int bid[SS_PPL];
#pragma unroll
    for (int j = 0; j < SS_PPL; ++j) {
        const long long i = p0 + tid * SS_PPL + j;
        bid[j] = -1;
#pragma unroll
        for (int l = 0; l < D; ++l) x[j][l] = 0.0f;
        if (i >= pe) continue;
        if constexpr (GRID) {
            long long rem = i;
            int idx[D];
#pragma unroll
            for (int l = D - 1; l >= 0; --l) {
                const long long q = rem / a.ext[l];
                idx[l] = (int)(rem - q * a.ext[l]);
                rem = q;
            }
            int b = 0;
#pragma unroll
            for (int l = 0; l < D; ++l) {
                x[j][l] = a.ax[l][idx[l]];
                b = b * a.grid[l] + min(max(a.ab[l][idx[l]], 0), a.grid[l] - 1);
            }
            bid[j] = b;
        } else {
            bool in = true;
            int b = 0;
#pragma unroll
            for (int l = 0; l < D; ++l) {
                const float xs = a.points[i * D + l];
                int g;
                float un;
                in = sample_resolve(xs, a.nbs[l], (float)a.shape[l], g, un) && in;
                b = b * a.grid[l] + g;
                x[j][l] = (a.shape[l] > 1) ? __fdiv_rn(xs - 0.5f, (float)(a.shape[l] - 1)) : 0.0f;
            }
            bid[j] = in ? b : -1;
        }
    }

    float S[SS_PPL], inv[SS_PPL], y[SS_PPL][C], best[SS_PPL];
    int arg[SS_PPL];
#pragma unroll
    for (int j = 0; j < SS_PPL; ++j) {
        S[j] = 0.0f;
        inv[j] = 0.0f;
        first_max_init(best[j], arg[j], -1);
#pragma unroll
        for (int c = 0; c < C; ++c) y[j][c] = 0.0f;
    }

    // ---- 2. the distinct batches of the workgroup's points, ascending ----
    int last = -1;                                                   // the batch just done
    for (;;) {
        int mine = SS_NONE;
#pragma unroll
        for (int j = 0; j < SS_PPL; ++j)
            if (bid[j] > last) mine = min(mine, bid[j]);
        if (tid == 0) { s_cnt[5] = SS_NONE; s_cnt[0] = 0; }
        __syncthreads();
        if (mine != SS_NONE) atomicMin(&s_cnt[5], mine);
        __syncthreads();
        const int cur = s_cnt[5];                                    // workgroup-uniform
        if (cur == SS_NONE) break;
        last = cur;

        // ---- 2a. compact the batch's kernel list: listed & pis > 0, ascending ids (step 0 of shared_render_kernel) ----
        // The same list as the render kernel's, made per list WORD: a workgroup here compacts once per batch it meets, not
        // once per launch, and a pruned list has a handful of set bits in K / 32 words -- one round for K <= 8192 instead of
        // K / 256 rounds of three barriers.  A lane takes a word, drops the bits whose prior is not > 0 (one load per set
        // bit), and writes its kernels behind those of the words before it (wave_scan + per-wavefront totals).
        const uint32_t* bits = (a.lists != nullptr) ? a.lists + (size_t)cur * a.KW : nullptr;
        for (int wbase = 0; wbase < a.KW; wbase += SH_THREADS) {
            const int w = wbase + tid;
            uint32_t word = 0u;
            if (w < a.KW) {
                word = (bits != nullptr) ? bits[w] : 0xffffffffu;
                const int left = K - w * 32;                         // kernels from this word on (> 0)
                if (left < 32) word &= (1u << left) - 1u;
                for (uint32_t m = word; m != 0u; m &= m - 1u) {
                    const int bit = __ffs((int)m) - 1;
                    if (!(fqv(a.p.pis[w * 32 + bit], a.kc, 3) > 0.0f)) word &= ~(1u << bit);
                }
            }
            const int cnt = __popc(word);
            const int incl = wave_scan(cnt);                         // kernels of this wavefront's words up to this lane's
            if (lane == 63) s_cnt[1 + wave] = incl;
            __syncthreads();
            int off = s_cnt[0] + incl - cnt;
            for (int ww = 0; ww < wave; ++ww) off += s_cnt[1 + ww];
            for (; word != 0u; word &= word - 1u) s_list[off++] = w * 32 + __ffs((int)word) - 1;
            __syncthreads();
            if (tid == 0) s_cnt[0] += s_cnt[1] + s_cnt[2] + s_cnt[3] + s_cnt[4];
            __syncthreads();
        }
        const int Kact = s_cnt[0];

        int staged_c0 = -1;
        auto stage = [&](int c0, int n) {
            if (c0 == staged_c0) return;
            staged_c0 = c0;
            __syncthreads();
            if (tid < n) shared_stage_record<D, C, IC, false>(a.p, a.kc, a.qrng, a.mus_grid, s_list[c0 + tid], s_par + tid * L::SP);
            __syncthreads();
        };

        // ---- 2b. sweep A: gate normaliser ----
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
#pragma unroll
                for (int j = 0; j < SS_PPL; ++j) {
                    if (bid[j] != cur) continue;
                    float z[D];
                    S[j] += shared_gate<D, C, IC>(r, x[j], z);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SS_PPL; ++j)
            if (bid[j] == cur) inv[j] = frcp(fmaxf(S[j], 10e-12f));

        // ---- 2c. sweep B: masked gate, experts, blend, first maximum ----
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
                const int kid = s_list[c0 + kk];
#pragma unroll
                for (int j = 0; j < SS_PPL; ++j) {
                    if (bid[j] != cur) continue;
                    float z[D];
                    const float w = shared_gate<D, C, IC>(r, x[j], z) * inv[j];
                    const float wt = (w > a.kc.tau) ? w : 0.0f;
                    first_max_take(best[j], arg[j], wt, kid);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        float ee = r[L::O_NU + c];
#pragma unroll
                        for (int l = 0; l < D; ++l) ee = fmaf(r[L::O_GA + l * C + c], x[j][l], ee);
                        y[j][c] = fmaf(wt, ee, y[j][c]);
                    }
                }
            }
        }
        // (the next round begins with a barrier before anything of this batch in LDS is overwritten)
    }

    // ---- 3. clip + 8-bit lattice (the output stage of shared_render_kernel), through LDS to the dense planes ----
#pragma unroll
    for (int j = 0; j < SS_PPL; ++j) {
        const int si = tid * SS_PPL + j;
        if (p0 + si >= pe) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float yc = __builtin_amdgcn_fmed3f(y[j][c], 0.0f, a.kc.nudged_max);
            const float kq = (bid[j] >= 0) ? floorf(fmaf(yc, a.kc.inv_scale, 0.5f)) : 0.0f;
            s_val[si * C + c] = (a.fmt == SMOE_IMAGE_U8) ? (uint32_t)kq : __float_as_uint(kq * a.kc.scale);
        }
        s_arg[si] = (uint32_t)((bid[j] >= 0) ? arg[j] : -1);
    }
    __syncthreads();
    const int vs_img = a.vec_img ? ((a.fmt == SMOE_IMAGE_U8) ? 4 : 2) : 0;       // log2 of the elements per 16-byte store
    const int vs_arg = a.vec_arg ? 2 : 0;
    for (int plane = 0; plane < 2; ++plane) {
        if (plane == 1 && a.argmax == nullptr) continue;
        const int cps = (plane == 0) ? C : 1;
        const int vs = (plane == 0) ? vs_img : vs_arg;
        const int cpr = ((SS_TILE * cps + (1 << vs) - 1) >> vs) + 1;             // 16-byte lines the run can touch
        const long long e0 = p0 * cps, e1 = pe * cps;
        for (int ch = tid; ch < cpr; ch += SH_THREADS) {
            if (plane == 1) render_store_run<false>(s_arg, a.argmax, e0, e1, 0, vs, ch);
            else if (a.fmt == SMOE_IMAGE_U8) render_store_run<true>(s_val, a.image, e0, e1, 0, vs, ch);
            else render_store_run<false>(s_val, a.image, e0, e1, 0, vs, ch);
        }
    }
}

// The launch geometry and the LDS need of a call for checked arguments: pure host code.  hipErrorNotSupported: 2^31 or more
// workgroups, or more than 160 KB of LDS.
hipError_t shared_sample_layout(int D, int C, int K, long long num_points, RenderLayout& g) {
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    g.hl = 0;
    g.lds_bytes = sizeof(float) * (((size_t)K + (size_t)SH_KC * SP + 8 + (size_t)SS_TILE * (C + 1) + 3) & ~(size_t)3);
    g.workgroups = (num_points + SS_TILE - 1) / SS_TILE;
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    if (g.workgroups > 0x7fffffffLL) return hipErrorNotSupported;
    return hipSuccess;
}

template <int D, int C>
static hipError_t launch_shared_sample_dc(const SharedSampleArgs& a, bool grid, const RenderLayout& g, hipStream_t st) {
    const bool ic = a.kc.inverse_cov != 0;
    auto kern = grid ? (ic ? shared_sample_kernel<D, C, true, true> : shared_sample_kernel<D, C, false, true>)
                     : (ic ? shared_sample_kernel<D, C, true, false> : shared_sample_kernel<D, C, false, false>);
    return launch_decoder(kern, g.workgroups, SH_THREADS, g.lds_bytes, a, st);
}

// The kernel of a planned call (g from shared_sample_layout): the launch alone.  grid: the points are the dense view of a.ext
// with the per-axis tables a.ax / a.ab, otherwise the list a.points.
hipError_t launch_shared_sample(const SharedSampleArgs& a, int D, int C, bool grid, const RenderLayout& g, hipStream_t st) {
    if (D == 2 && C == 1) return launch_shared_sample_dc<2, 1>(a, grid, g, st);
    if (D == 2 && C == 3) return launch_shared_sample_dc<2, 3>(a, grid, g, st);
    if (D == 3 && C == 1) return launch_shared_sample_dc<3, 1>(a, grid, g, st);
    if (D == 3 && C == 3) return launch_shared_sample_dc<3, 3>(a, grid, g, st);
    return hipErrorInvalidValue;
}

}  // namespace smoe
#endif
