// smoe_shared_sample_area_each.hip.h -- anti-aliased point decoder of the shared-kernel image mode with a footprint and tap
// counts of its own for every point (smoe_shared_sample_area_each, include/smoe_hip.h): smoe_shared_sample_area for views whose
// magnification varies across the output -- a perspective view, a lens map, any dense lookup map of a whole-image model.
// Included by smoe_shared.hip after smoe_shared_sample_area.hip.h; it calls shared_stage_record, shared_gate, sample_resolve,
// wave_scan and render_store_run and changes none.
//
// Definition.  Point i has the centre x = points[i], the footprint F = footprints[i] ([d, d] row-major, source pixels) and the
// tap counts n = taps[i] (a byte per view axis).  Its result is that of smoe_shared_sample_area (smoe_shared_sample_area.hip.h)
// called with this one point, this footprint and these taps, bit for bit: per tap multi-index j, all in IEEE fp32,
//     offset     o_m = (float)(2 j_m + 1 - n_m) / (float)(2 n_m)
//     position   t_l = x_l, then for m = 0 .. d-1: t_l = t_l + (F[l][m] * o_m)      product and sum rounded separately
//     value, mean, outputs: word for word as there (the list of the batch the TAP lies in, row-major order of j, inside taps
//     only, one division, the lattice with its fminf clamp, batch = the batch of the centre, no argmax).
// A point is VOID if a tap count is outside 1 .. 16, if their product is above 64 or if an entry of its footprint is not finite
// (smoe_sample_area_each's rule): values 0, mean 0, count 0, batch = the centre's batch as for every point.  The host cannot
// read the device arrays, so this is a defined result and not an error; a void point has no item (T = 0, every other point's at
// most 64, whatever bytes the arrays hold).  A point owes nothing to the other points, its place in the list or how the launch
// is cut.
//
// Arrangement.  smoe_sample_area_each lets one lane walk its own taps, because a tap there needs its block's record only.
// Here a tap needs the compacted kernel list of the batch it lies in, so the taps are the parallel items of
// shared_sample_area_kernel's cooperative walk -- and the number of items per point is device data.
//  * Fixed point runs.  A workgroup of 256 lanes takes SSE_POINTS consecutive points, so the host plans the grid without
//    reading device data: ceil(N / SSE_POINTS) workgroups.
//  * Prologue.  Lane p < np loads its point's centre, footprint and tap bytes with plain per-lane loads (any alignment; a copy)
//    into LDS slots, decides void and scans T_p (0 for void): one wave_scan per wavefront plus the wave totals give the
//    exclusive prefix s_off[0 .. SSE_POINTS] (T = 0 past np) and the item total M = s_off[SSE_POINTS] <= 64 SSE_POINTS.
//  * Rounds.  R = ceil(M / SSE_TILE), SSE_TILE = 256 SSE_PPL, workgroup-uniform (read from LDS); SSE_PPL, the items per lane
//    and round, is 1 on two axes and 2 on three (sse_ppl below).  In round r a lane's item
//    v = r SSE_TILE + tid SSE_PPL + j (idle from M on) finds its point by a binary search in s_off (log2 SSE_POINTS steps; a
//    lane's next item first looks whether it is still inside the point of the one before), its multi-index by divisions by
//    that point's n_m, its offsets in the 256-entry table s_tab[(n - 1) * 16 + j] of smoe_sample_area_each (one __fdiv_rn per
//    entry) and its position from the point's LDS slot.  From there a round is shared_sample_area_kernel's section 2: the
//    walk over the distinct batches of the round's items in ascending id (LDS atomicMin, list compacted per word, records in
//    chunks of SH_KC, sweeps A and B); then each item's clipped V and inside flag go into the staging.
//  * Owners across rounds.  The owner of point p is lane p; it keeps acc[C] and cnt in registers across the rounds and, after
//    each round's barrier, adds those of its taps that lie in this round's item range in ascending item order.  Rounds ascend
//    and items ascend within a round, so the order is the row-major one wherever the round boundaries fall.  Item w of the
//    round, of point p, is staged at w (C + 1) + p dwords: a point's run starts T (C + 1) + 1 dwords behind the one before
//    (an odd number, shared_sample_area_kernel's stride), so owners with equal tap counts do not meet in one LDS bank.
//  * Epilogue.  After the last round the owner forms mean, lattice value and the centre's batch; the four planes are staged
//    where the taps were (behind a barrier) and leave through render_store_run as there: 64-bit element offsets.
// No inline assembly; the only atomics are LDS int; every barrier is reached by all 256 lanes (trip counts depend on M, K and
// the batch only, all read from LDS or arguments).
// The walker's statements are repeated here a fourth time (after shared_sample_kernel, shared_sample_grad_kernel and
// shared_sample_area_kernel), so that those three stay byte for byte with their resource figures: DESIGN 8 lists it as debt.
#ifndef SMOE_SHARED_SAMPLE_AREA_EACH_HIP_H
#define SMOE_SHARED_SAMPLE_AREA_EACH_HIP_H

#include "smoe_shared_sample_area.hip.h"

namespace smoe {

#ifndef SMOE_SSE_POINTS
#define SMOE_SSE_POINTS 64
#endif
#ifndef SMOE_SSE_PPL2
#define SMOE_SSE_PPL2 1
#endif
#ifndef SMOE_SSE_PPL3
#define SMOE_SSE_PPL3 2
#endif
constexpr int SSE_POINTS = SMOE_SSE_POINTS;              // points per workgroup
// items (taps) per lane and round, by the number of axes: one on two axes (the faster of the two where both were timed), two on
// three (with one the d = 3 instantiations come out with a 36-byte private segment per lane)
__host__ __device__ constexpr int sse_ppl(int D) { return (D == 2) ? SMOE_SSE_PPL2 : SMOE_SSE_PPL3; }
__host__ __device__ constexpr int sse_tile(int D) { return SH_THREADS * sse_ppl(D); }      // items per round
static_assert(SSE_POINTS >= 1 && SSE_POINTS <= SH_THREADS && (SSE_POINTS & (SSE_POINTS - 1)) == 0,
              "one owner lane per point; the search in s_off halves a power of two");
static_assert(SH_THREADS == SSA_AT * SSA_AT, "one lane per entry of the offset table");

// staging dwords of a workgroup: a round's V and flag (one pad dword per point), later the four output planes
__host__ __device__ inline int sse_stage_dwords(int D, int C) {
    const int taps = sse_tile(D) * (C + 1) + SSE_POINTS;
    const int outs = SSE_POINTS * (2 * C + 2);
    return (taps > outs) ? taps : outs;
}

template <int D, int C, bool IC>
__global__ void __launch_bounds__(SH_THREADS) shared_sample_area_each_kernel(SharedSampleAreaEachArgs q) {
    using L = SL<D, C>;
    constexpr int NP = SSE_POINTS;
    constexpr int SSE_PPL = sse_ppl(D);
    constexpr int SSE_TILE = sse_tile(D);
    const SharedSampleArgs& a = q.s;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int K = a.K;
    const long long p0 = (long long)blockIdx.x * NP;                   // the workgroup's first point
    const long long pe = (a.num_points - p0 < NP) ? a.num_points : p0 + NP;
    const int np = (int)(pe - p0);                                     // its points, 1 .. NP

    // LDS carve-up (shared_sample_area_each_layout)
    int* s_list = reinterpret_cast<int*>(lds);                       // [K] compacted active kernel ids of the current batch
    float* s_par = lds + K;                                          // [SH_KC][SP]
    int* s_cnt = reinterpret_cast<int*>(s_par + SH_KC * L::SP);      // [8]: 0 list length, 1..4 per wavefront, 5 next batch
    float* s_tab = reinterpret_cast<float*>(s_cnt + 8);              // [16][16] o(n, j), 0 past n
    float* s_fp = s_tab + SSA_AT * SSA_AT;                           // [NP][D * D] footprints
    float* s_x = s_fp + NP * D * D;                                  // [NP][D] centres
    int* s_nt = reinterpret_cast<int*>(s_x + NP * D);                // [NP] tap counts, a byte per axis (1 .. 16; void: unused)
    int* s_off = s_nt + NP;                                          // [NP + 1] exclusive prefix of the points' item counts
    uint32_t* s_stg = reinterpret_cast<uint32_t*>(s_off + NP + 4);   // sse_stage_dwords

    // ---- 0. prologue: the offset table, the points' slots, the prefix of their item counts ----
    {
        const int n = (tid >> 4) + 1, j = tid & (SSA_AT - 1);
        s_tab[tid] = (j < n) ? __fdiv_rn((float)(2 * j + 1 - n), (float)(2 * n)) : 0.0f;
    }
    int T = 0;                                                         // the lane's point: its items (void, or no point: 0)
    if (tid < np) {
        const long long i = p0 + tid;
        bool ok = true;
        int prod = 1, packed = 0;
#pragma unroll
        for (int m = 0; m < D; ++m) {
            const int n = q.taps[i * D + m];
            ok = ok && n >= 1 && n <= SSA_AT;
            prod *= ok ? n : 1;
            packed |= n << (8 * m);
        }
        ok = ok && prod <= SAMPLE_AREA_TAPS;
#pragma unroll
        for (int e = 0; e < D * D; ++e) {
            const float f = q.footprints[i * (D * D) + e];
            ok = ok && (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u;
            s_fp[tid * (D * D) + e] = f;
        }
#pragma unroll
        for (int l = 0; l < D; ++l) s_x[tid * D + l] = a.points[i * D + l];
        s_nt[tid] = packed;
        T = ok ? min(prod, SAMPLE_AREA_TAPS) : 0;
    }
    {
        const int incl = wave_scan(T);
        if (lane == 63) s_cnt[1 + wave] = incl;
        __syncthreads();
        int off = incl;
        for (int ww = 0; ww < wave; ++ww) off += s_cnt[1 + ww];
        if (tid < NP) s_off[tid + 1] = off;
        if (tid == 0) s_off[0] = 0;
        __syncthreads();                                             // (also publishes s_tab and the slots)
    }
    const int my0 = (tid < NP) ? s_off[tid] : 0;                     // the owner's items [my0, my1)
    const int my1 = (tid < NP) ? s_off[tid + 1] : 0;
    const int M = s_off[NP];                                         // workgroup-uniform, <= 64 NP
    const int R = (M + SSE_TILE - 1) / SSE_TILE;

    float acc[C];                                                      // the owner's ordered sum and count, across the rounds
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    int cnt = 0;

    for (int r = 0; r < R; ++r) {
        const int v0 = r * SSE_TILE;
        // ---- 1. this lane's items: point, tap position, image-unit coordinates and owning batch (-1: outside, or idle) ----
        float x[SSE_PPL][D];
        int bid[SSE_PPL], ipt[SSE_PPL];
        int prev = -1;
#pragma unroll
        for (int j = 0; j < SSE_PPL; ++j) {
            const int v = v0 + tid * SSE_PPL + j;
            bid[j] = -1;
            ipt[j] = -1;
#pragma unroll
            for (int l = 0; l < D; ++l) x[j][l] = 0.0f;
            if (v >= M) continue;
            int pi;                                                  // s_off[pi] <= v < s_off[pi + 1]
            if (prev >= 0 && v < s_off[prev + 1]) {
                pi = prev;
            } else {
                pi = 0;                                              // the entries of s_off[1 .. NP] that are <= v: at most NP - 1
#pragma unroll
                for (int step = NP / 2; step >= 1; step >>= 1)
                    if (s_off[pi + step] <= v) pi += step;
            }
            prev = pi;
            ipt[j] = pi;
            const int packed = s_nt[pi];
            int rem = v - s_off[pi];                                 // the tap's index, last axis fastest; 0 <= rem < T_pi <= 64
            float om[D];
#pragma unroll
            for (int m = D - 1; m >= 0; --m) {
                const int n = (packed >> (8 * m)) & 0xff;            // 1 .. 16: the point is not void
                const int qq = rem / n;
                om[m] = s_tab[(n - 1) * SSA_AT + (rem - qq * n)];
                rem = qq;
            }
            const float* Fs = s_fp + pi * (D * D);
            bool in = true;
            int b = 0;
#pragma unroll
            for (int l = 0; l < D; ++l) {
                float xs = s_x[pi * D + l];
#pragma unroll
                for (int m = 0; m < D; ++m) xs = __fadd_rn(xs, __fmul_rn(Fs[l * D + m], om[m]));
                int g;
                float un;
                in = sample_resolve(xs, a.nbs[l], (float)a.shape[l], g, un) && in;
                b = b * a.grid[l] + g;
                x[j][l] = (a.shape[l] > 1) ? __fdiv_rn(xs - 0.5f, (float)(a.shape[l] - 1)) : 0.0f;
            }
            bid[j] = in ? b : -1;
        }

        float S[SSE_PPL], inv[SSE_PPL], y[SSE_PPL][C];
#pragma unroll
        for (int j = 0; j < SSE_PPL; ++j) {
            S[j] = 0.0f;
            inv[j] = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) y[j][c] = 0.0f;
        }

        // ---- 2. the distinct batches of the round's items, ascending (the walk of shared_sample_kernel) ----
        int last = -1;                                               // the batch just done
        for (;;) {
            int mine = SS_NONE;
#pragma unroll
            for (int j = 0; j < SSE_PPL; ++j)
                if (bid[j] > last) mine = min(mine, bid[j]);
            if (tid == 0) { s_cnt[5] = SS_NONE; s_cnt[0] = 0; }
            __syncthreads();
            if (mine != SS_NONE) atomicMin(&s_cnt[5], mine);
            __syncthreads();
            const int cur = s_cnt[5];                                // workgroup-uniform
            if (cur == SS_NONE) break;
            last = cur;

            // ---- 2a. compact the batch's kernel list per list word: listed & pis > 0, ascending ids ----
            const uint32_t* bits = (a.lists != nullptr) ? a.lists + (size_t)cur * a.KW : nullptr;
            for (int wbase = 0; wbase < a.KW; wbase += SH_THREADS) {
                const int w = wbase + tid;
                uint32_t word = 0u;
                if (w < a.KW) {
                    word = (bits != nullptr) ? bits[w] : 0xffffffffu;
                    const int left = K - w * 32;                     // kernels from this word on (> 0)
                    if (left < 32) word &= (1u << left) - 1u;
                    for (uint32_t m = word; m != 0u; m &= m - 1u) {
                        const int bit = __ffs((int)m) - 1;
                        if (!(fqv(a.p.pis[w * 32 + bit], a.kc, 3) > 0.0f)) word &= ~(1u << bit);
                    }
                }
                const int nk = __popc(word);
                const int incl = wave_scan(nk);                      // kernels of this wavefront's words up to this lane's
                if (lane == 63) s_cnt[1 + wave] = incl;
                __syncthreads();
                int off = s_cnt[0] + incl - nk;
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
                    const float* rr = s_par + kk * L::SP;
#pragma unroll
                    for (int j = 0; j < SSE_PPL; ++j) {
                        if (bid[j] != cur) continue;
                        float z[D];
                        S[j] += shared_gate<D, C, IC>(rr, x[j], z);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < SSE_PPL; ++j)
                if (bid[j] == cur) inv[j] = frcp(fmaxf(S[j], 10e-12f));

            // ---- 2c. sweep B: masked gate, experts, blend ----
            for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
                const int n = min(SH_KC, Kact - c0);
                stage(c0, n);
                for (int kk = 0; kk < n; ++kk) {
                    const float* rr = s_par + kk * L::SP;
#pragma unroll
                    for (int j = 0; j < SSE_PPL; ++j) {
                        if (bid[j] != cur) continue;
                        float z[D];
                        const float w = shared_gate<D, C, IC>(rr, x[j], z) * inv[j];
                        const float wt = (w > a.kc.tau) ? w : 0.0f;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            float ee = rr[L::O_NU + c];
#pragma unroll
                            for (int l = 0; l < D; ++l) ee = fmaf(rr[L::O_GA + l * C + c], x[j][l], ee);
                            y[j][c] = fmaf(wt, ee, y[j][c]);
                        }
                    }
                }
            }
            // (the next turn begins with a barrier before anything of this batch in LDS is overwritten)
        }

        // ---- 3. the items' clipped values and inside flags into the staging (the walk's barriers lie between the owners'
        //         reads of the round before and these writes) ----
#pragma unroll
        for (int j = 0; j < SSE_PPL; ++j) {
            if (ipt[j] < 0) continue;
            uint32_t* st = s_stg + (tid * SSE_PPL + j) * (C + 1) + ipt[j];
#pragma unroll
            for (int c = 0; c < C; ++c) st[c] = __float_as_uint(__builtin_amdgcn_fmed3f(y[j][c], 0.0f, a.kc.nudged_max));
            st[C] = (bid[j] >= 0) ? 1u : 0u;
        }
        __syncthreads();

        // ---- 4. the owner of a point adds those of its taps that lie in this round, in ascending item order ----
        {
            const int w0 = max(my0, v0) - v0, w1 = min(my1, v0 + SSE_TILE) - v0;
            const uint32_t* st = s_stg + tid;                        // (w0 < w1 for owners tid < NP only)
            for (int w = w0; w < w1; ++w) {
                if (st[w * (C + 1) + C] != 0u) {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], __uint_as_float(st[w * (C + 1) + c]));
                    ++cnt;
                }
            }
        }
    }

    // ---- 5. epilogue: the mean, the lattice value, the centre's batch; the four planes ----
    float om[C], ov[C];
    int ob = -1;
    const float kmax = floorf(fmaf(a.kc.nudged_max, a.kc.inv_scale, 0.5f));     // the index of the clip's upper end
#pragma unroll
    for (int c = 0; c < C; ++c) { om[c] = 0.0f; ov[c] = 0.0f; }
    if (tid < np) {
        bool cin = true;
        int cb = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            int g;
            float un;
            cin = sample_resolve(s_x[tid * D + l], a.nbs[l], (float)a.shape[l], g, un) && cin;
            cb = cb * a.grid[l] + g;
        }
        ob = cin ? cb : -1;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            om[c] = (cnt > 0) ? __fdiv_rn(acc[c], (float)cnt) : 0.0f;
            ov[c] = fminf(floorf(fmaf(om[c], a.kc.inv_scale, 0.5f)), kmax);
        }
    }
    __syncthreads();                                                 // every tap is read: the planes take the staging's place
    uint32_t* s_val = s_stg;                                         // [NP][C] lattice values / indices
    uint32_t* s_mean = s_val + NP * C;                               // [NP][C] mean bits
    uint32_t* s_num = s_mean + NP * C;                               // [NP] counts
    uint32_t* s_bid = s_num + NP;                                    // [NP] batch ids of the centres
    if (tid < np) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            s_val[tid * C + c] = (a.fmt == SMOE_IMAGE_U8) ? (uint32_t)ov[c] : __float_as_uint(ov[c] * a.kc.scale);
            s_mean[tid * C + c] = __float_as_uint(om[c]);
        }
        s_num[tid] = (uint32_t)cnt;
        s_bid[tid] = (uint32_t)ob;
    }
    __syncthreads();
    const bool u8 = a.fmt == SMOE_IMAGE_U8;
    for (int plane = 0; plane < 4; ++plane) {
        const uint32_t* st = (plane == 0) ? s_val : ((plane == 1) ? s_mean : ((plane == 2) ? s_num : s_bid));
        void* dst = (plane == 0) ? a.image : ((plane == 1) ? (void*)q.mean : ((plane == 2) ? (void*)q.count : (void*)q.batch));
        if (dst == nullptr) continue;
        const int cps = (plane < 2) ? C : 1;
        const bool bytes = (plane == 0) ? u8 : (plane == 2);
        const int vec = (plane == 0) ? a.vec_img : ((plane == 1) ? q.vec_mean : ((plane == 2) ? q.vec_cnt : q.vec_bat));
        const int vs = vec ? (bytes ? 4 : 2) : 0;                                // log2 of the elements per 16-byte store
        const int cpr = ((NP * cps + (1 << vs) - 1) >> vs) + 1;                  // 16-byte lines the run can touch
        const long long e0 = p0 * cps, e1 = pe * cps;
        for (int ch = tid; ch < cpr; ch += SH_THREADS) {
            if (bytes) render_store_run<true>(st, dst, e0, e1, 0, vs, ch);
            else render_store_run<false>(st, dst, e0, e1, 0, vs, ch);
        }
    }
}

// The launch geometry and the LDS need of a call for checked arguments: pure host code, no device data is read (a workgroup
// takes SSE_POINTS points whatever their tap counts).  g.hl is unused and 0.  hipErrorNotSupported: 2^31 or more workgroups,
// or more than 160 KB of LDS.
hipError_t shared_sample_area_each_layout(int D, int C, int K, long long num_points, RenderLayout& g) {
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    g.hl = 0;
    g.lds_bytes = sizeof(float) * (((size_t)K + (size_t)SH_KC * SP + 8 + (size_t)(SSA_AT * SSA_AT)
                                    + (size_t)SSE_POINTS * (D * D + D + 1) + (size_t)(SSE_POINTS + 4)
                                    + (size_t)sse_stage_dwords(D, C) + 3) & ~(size_t)3);
    g.workgroups = num_points / SSE_POINTS + ((num_points % SSE_POINTS != 0) ? 1 : 0);
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    if (g.workgroups > 0x7fffffffLL) return hipErrorNotSupported;
    return hipSuccess;
}

template <int D, int C>
static hipError_t launch_shared_sample_area_each_dc(const SharedSampleAreaEachArgs& q, const RenderLayout& g, hipStream_t st) {
    const bool ic = q.s.kc.inverse_cov != 0;
    auto kern = ic ? shared_sample_area_each_kernel<D, C, true> : shared_sample_area_each_kernel<D, C, false>;
    return launch_decoder(kern, g.workgroups, SH_THREADS, g.lds_bytes, q, st);
}

// The kernel of a planned call (g from shared_sample_area_each_layout): the launch alone.
hipError_t launch_shared_sample_area_each(const SharedSampleAreaEachArgs& q, int D, int C, const RenderLayout& g, hipStream_t st) {
    if (D == 2 && C == 1) return launch_shared_sample_area_each_dc<2, 1>(q, g, st);
    if (D == 2 && C == 3) return launch_shared_sample_area_each_dc<2, 3>(q, g, st);
    if (D == 3 && C == 1) return launch_shared_sample_area_each_dc<3, 1>(q, g, st);
    if (D == 3 && C == 3) return launch_shared_sample_area_each_dc<3, 3>(q, g, st);
    return hipErrorInvalidValue;
}

}  // namespace smoe
#endif
