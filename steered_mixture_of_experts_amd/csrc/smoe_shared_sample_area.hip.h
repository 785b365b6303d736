// smoe_shared_sample_area.hip.h -- anti-aliased point decoder of the shared-kernel image mode: the mean of the ONE global
// kernel set over a small regular grid of taps inside the footprint of every output sample, every tap with the kernel list of
// the batch that owns IT, [N, C] (smoe_shared_sample_area, include/smoe_hip.h) -- smoe_sample_area for a whole-image model.
// Included by smoe_shared.hip after smoe_shared_sample_grad.hip.h; it calls shared_stage_record, shared_gate, sample_resolve
// and render_store_run and changes none.
//
// Definition.  A point x is the centre of an output cell, in source pixels as for smoe_shared_sample.  The footprint F [d, d]
// (row-major, source pixels) holds in column m the edge vector of the cell along view axis m; taps[m] (1 .. 16, product at most
// 64) is the number of taps along that axis.  One footprint serves all points of a call.  Per point and tap multi-index j, all
// in IEEE fp32:
//     offset     o_m = (float)(2 j_m + 1 - taps[m]) / (float)(2 taps[m])        an exact integer numerator, one rounded division
//     position   t_l = x_l, then for m = 0 .. d-1: t_l = t_l + (F[l][m] * o_m)   product and sum rounded separately, no fma:
//                smoe_sample_area's, blocks.area_taps gives it bit for bit
//     value      the tap is resolved exactly as a point of smoe_shared_sample_grad: the outside rule against image_shape, the
//                owning batch from sample_resolve, u = __fdiv_rn(t - 0.5f, (float)(S - 1)) (0 for S == 1), the compacted list
//                of THAT batch (listed, fake-quantised prior > 0, ascending ids; lists == NULL: every kernel), sweeps A and B
//                and the clip as the same statements in the same order; its value is that call's `values` V, bit for bit
//     mean       acc_c = 0, cnt = 0; over the taps in row-major order of j (last axis fastest) an inside tap adds
//                acc_c = acc_c + V_c (one fp32 add) and cnt += 1; mean_c = __fdiv_rn(acc_c, (float)cnt); cnt == 0: 0.
//                Taps outside the image are left out, not counted as black.  The order is smoe_sample_area's and does not
//                depend on which batches the taps fall in.
// Outputs: values = the mean put on the lattice by the statement shared_sample_kernel ends with, floorf(fmaf(v, inv_scale, 0.5f)),
// times scale for F32, the index for U8 -- with one tap smoe_shared_sample's image bit for bit; mean; count = cnt; batch = the
// global id of the batch that owns the CENTRE, -1 where the centre is outside (its taps inside still give their mean).  Every
// V is at most nudged_max, but the rounded sum of up to 64 of them over their count may pass nudged_max by a few ulp; the index
// is therefore clamped to the one of nudged_max (no change wherever the mean is within the clip).  No argmax: an average has no
// single kernel.  A point's result depends on its coordinates, the footprint, the taps, the model and the lists of the batches
// its taps lie in only: not on N, its place in the list, the other points or the cut of the launch.
//
// Arrangement.  The taps are the parallel items.  With T = prod(taps), a workgroup of 256 lanes takes P = SSA_TILE / T
// consecutive points; lane t takes the SSA_PPL consecutive items v from t * SSA_PPL on, item v being tap v % T of point v / T
// (items past P T or past the last point are idle, batch -1).  The products F[l][m] * o_m go once per workgroup into an LDS
// table [d][d][16] (sample_area_kernel's); a lane forms its taps' positions from the centre with __fadd_rn and resolves them
// with sample_resolve.  From there the kernel is shared_sample_kernel's walk over the DISTINCT batches of the workgroup's
// items in ascending id (LDS atomicMin, list compacted per word, records in chunks of SH_KC, sweeps A and B), an item's S, inv
// and y[C] in registers -- a cell that straddles batches simply has items in several rounds, and a list longer than one chunk
// needs nothing new.  After the walk every lane writes its items' clipped V and an inside flag to LDS; after one barrier the
// owner of point p (p = tid, tid + 256, ...) adds its T taps in row-major order, forms cnt, the mean and the lattice value and
// resolves the centre's batch; the four output planes are staged where the taps were (behind a barrier) and leave as one dense
// run per plane (render_store_run): 16-byte non-temporal stores where the plane's base is 16-byte aligned, element-wise at the
// ragged head and tail, 64-bit element offsets.  A point's taps are staged T (C + 1) + 1 dwords apart, an odd number, so the
// owners' reads do not meet in one LDS bank.  No inline assembly; the only atomics are LDS int; every barrier is reached by
// all 256 lanes (trip counts depend on K, T and the batch only).
// The walker's statements are repeated here a third time (after shared_sample_kernel and shared_sample_grad_kernel), so that
// those two stay byte for byte with their resource figures: DESIGN 8 lists it as debt.
#ifndef SMOE_SHARED_SAMPLE_AREA_HIP_H
#define SMOE_SHARED_SAMPLE_AREA_HIP_H

#include "smoe_shared_sample_grad.hip.h"

namespace smoe {

#ifndef SMOE_SSA_PPL
#define SMOE_SSA_PPL 2
#endif
constexpr int SSA_PPL = SMOE_SSA_PPL;                    // items (taps) per lane
constexpr int SSA_TILE = SH_THREADS * SSA_PPL;           // items per workgroup
constexpr int SSA_AT = SAMPLE_AREA_AXIS_TAPS;

// staging dwords of a workgroup: the taps' V and flag (a point's taps one odd stride apart), later the four output planes
__host__ __device__ inline int ssa_stage_dwords(int C, int T, int P) {
    const int taps = P * (T * (C + 1) + 1);
    const int outs = P * (2 * C + 2);
    return (taps > outs) ? taps : outs;
}

template <int D, int C, bool IC>
__global__ void __launch_bounds__(SH_THREADS) shared_sample_area_kernel(SharedSampleAreaArgs q) {
    using L = SL<D, C>;
    const SharedSampleArgs& a = q.s;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int K = a.K;
    const int T = q.ntaps;
    const int P = q.ppw;                                               // points per workgroup, SSA_TILE / T
    const long long p0 = (long long)blockIdx.x * P;                    // the workgroup's first point
    const long long pe = (a.num_points - p0 < P) ? a.num_points : p0 + P;
    const int np = (int)(pe - p0);                                     // its points, 1 .. P

    // LDS carve-up (shared_sample_area_layout)
    int* s_list = reinterpret_cast<int*>(lds);                       // [K] compacted active kernel ids of the current batch
    float* s_par = lds + K;                                          // [SH_KC][SP]
    int* s_cnt = reinterpret_cast<int*>(s_par + SH_KC * L::SP);      // [8]: 0 list length, 1..4 per wavefront, 5 next batch
    float* s_tap = reinterpret_cast<float*>(s_cnt + 8);              // [D][D][16] F[l][m] * o_m(j), 0 past taps[m]
    uint32_t* s_stg = reinterpret_cast<uint32_t*>(s_tap + D * D * SSA_AT);   // ssa_stage_dwords
    const int pstride = T * (C + 1) + 1;                             // dwords from a point's taps to the next point's

    if (tid < SSA_AT) {
#pragma unroll
        for (int m = 0; m < D; ++m) {
            const int nt = q.taps[m];
            const float o = (tid < nt) ? __fdiv_rn((float)(2 * tid + 1 - nt), (float)(2 * nt)) : 0.0f;
#pragma unroll
            for (int l = 0; l < D; ++l) s_tap[(l * D + m) * SSA_AT + tid] = __fmul_rn(q.F[l * D + m], o);
        }
    }
    __syncthreads();

    // ---- 1. this lane's items: tap position, image-unit coordinates and owning batch (-1: outside, or idle) ----
    float x[SSA_PPL][D];
    int bid[SSA_PPL];
#pragma unroll
    for (int j = 0; j < SSA_PPL; ++j) {
        const int v = tid * SSA_PPL + j;
        const int pi = v / T;                                        // the item's point within the workgroup
        bid[j] = -1;
#pragma unroll
        for (int l = 0; l < D; ++l) x[j][l] = 0.0f;
        if (pi >= np) continue;
        int rem = v - pi * T, jm[D];                                 // the tap's multi-index, last axis fastest
#pragma unroll
        for (int m = D - 1; m >= 0; --m) {
            const int qq = rem / q.taps[m];
            jm[m] = rem - qq * q.taps[m];
            rem = qq;
        }
        const long long i = p0 + pi;
        bool in = true;
        int b = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            float xs = a.points[i * D + l];
#pragma unroll
            for (int m = 0; m < D; ++m) xs = __fadd_rn(xs, s_tap[(l * D + m) * SSA_AT + jm[m]]);
            int g;
            float un;
            in = sample_resolve(xs, a.nbs[l], (float)a.shape[l], g, un) && in;
            b = b * a.grid[l] + g;
            x[j][l] = (a.shape[l] > 1) ? __fdiv_rn(xs - 0.5f, (float)(a.shape[l] - 1)) : 0.0f;
        }
        bid[j] = in ? b : -1;
    }

    float S[SSA_PPL], inv[SSA_PPL], y[SSA_PPL][C];
#pragma unroll
    for (int j = 0; j < SSA_PPL; ++j) {
        S[j] = 0.0f;
        inv[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) y[j][c] = 0.0f;
    }

    // ---- 2. the distinct batches of the workgroup's items, ascending (the walk of shared_sample_kernel) ----
    int last = -1;                                                   // the batch just done
    for (;;) {
        int mine = SS_NONE;
#pragma unroll
        for (int j = 0; j < SSA_PPL; ++j)
            if (bid[j] > last) mine = min(mine, bid[j]);
        if (tid == 0) { s_cnt[5] = SS_NONE; s_cnt[0] = 0; }
        __syncthreads();
        if (mine != SS_NONE) atomicMin(&s_cnt[5], mine);
        __syncthreads();
        const int cur = s_cnt[5];                                    // workgroup-uniform
        if (cur == SS_NONE) break;
        last = cur;

        // ---- 2a. compact the batch's kernel list per list word: listed & pis > 0, ascending ids ----
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
                for (int j = 0; j < SSA_PPL; ++j) {
                    if (bid[j] != cur) continue;
                    float z[D];
                    S[j] += shared_gate<D, C, IC>(r, x[j], z);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SSA_PPL; ++j)
            if (bid[j] == cur) inv[j] = frcp(fmaxf(S[j], 10e-12f));

        // ---- 2c. sweep B: masked gate, experts, blend ----
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
#pragma unroll
                for (int j = 0; j < SSA_PPL; ++j) {
                    if (bid[j] != cur) continue;
                    float z[D];
                    const float w = shared_gate<D, C, IC>(r, x[j], z) * inv[j];
                    const float wt = (w > a.kc.tau) ? w : 0.0f;
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

    // ---- 3. the items' clipped values and inside flags into the tap staging (idle items of the workgroup's points: none) ----
#pragma unroll
    for (int j = 0; j < SSA_PPL; ++j) {
        const int v = tid * SSA_PPL + j;
        const int pi = v / T;
        if (pi >= np) continue;
        uint32_t* st = s_stg + pi * pstride + (v - pi * T) * (C + 1);
#pragma unroll
        for (int c = 0; c < C; ++c) st[c] = __float_as_uint(__builtin_amdgcn_fmed3f(y[j][c], 0.0f, a.kc.nudged_max));
        st[C] = (bid[j] >= 0) ? 1u : 0u;
    }
    __syncthreads();

    // ---- 4. the owner of a point: the ordered sum of its taps, the count, the mean, the lattice value, the centre's batch ----
    float om[SSA_PPL][C], ov[SSA_PPL][C];
    int oc[SSA_PPL], ob[SSA_PPL];
    const float kmax = floorf(fmaf(a.kc.nudged_max, a.kc.inv_scale, 0.5f));     // the index of the clip's upper end
#pragma unroll
    for (int j = 0; j < SSA_PPL; ++j) {
        const int pi = tid + j * SH_THREADS;
        oc[j] = 0;
        ob[j] = -1;
#pragma unroll
        for (int c = 0; c < C; ++c) { om[j][c] = 0.0f; ov[j][c] = 0.0f; }
        if (pi >= np) continue;
        const uint32_t* st = s_stg + pi * pstride;
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;
        int cnt = 0;
        for (int t = 0; t < T; ++t) {
            if (st[t * (C + 1) + C] != 0u) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], __uint_as_float(st[t * (C + 1) + c]));
                ++cnt;
            }
        }
        const long long i = p0 + pi;
        bool cin = true;
        int cb = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            int g;
            float un;
            cin = sample_resolve(a.points[i * D + l], a.nbs[l], (float)a.shape[l], g, un) && cin;
            cb = cb * a.grid[l] + g;
        }
        oc[j] = cnt;
        ob[j] = cin ? cb : -1;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            om[j][c] = (cnt > 0) ? __fdiv_rn(acc[c], (float)cnt) : 0.0f;
            ov[j][c] = fminf(floorf(fmaf(om[j][c], a.kc.inv_scale, 0.5f)), kmax);
        }
    }
    __syncthreads();                                                 // every tap is read: the planes take the staging's place
    uint32_t* s_val = s_stg;                                         // [P][C] lattice values / indices
    uint32_t* s_mean = s_val + P * C;                                // [P][C] mean bits
    uint32_t* s_num = s_mean + P * C;                                // [P] counts
    uint32_t* s_bid = s_num + P;                                     // [P] batch ids of the centres
#pragma unroll
    for (int j = 0; j < SSA_PPL; ++j) {
        const int pi = tid + j * SH_THREADS;
        if (pi >= np) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            s_val[pi * C + c] = (a.fmt == SMOE_IMAGE_U8) ? (uint32_t)ov[j][c] : __float_as_uint(ov[j][c] * a.kc.scale);
            s_mean[pi * C + c] = __float_as_uint(om[j][c]);
        }
        s_num[pi] = (uint32_t)oc[j];
        s_bid[pi] = (uint32_t)ob[j];
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
        const int cpr = ((P * cps + (1 << vs) - 1) >> vs) + 1;                   // 16-byte lines the run can touch
        const long long e0 = p0 * cps, e1 = pe * cps;
        for (int ch = tid; ch < cpr; ch += SH_THREADS) {
            if (bytes) render_store_run<true>(st, dst, e0, e1, 0, vs, ch);
            else render_store_run<false>(st, dst, e0, e1, 0, vs, ch);
        }
    }
}

// The launch geometry and the LDS need of a call for checked arguments (T = prod(taps), 1 .. 64): pure host code.  g.hl is
// unused and 0.  hipErrorNotSupported: 2^31 or more workgroups, or more than 160 KB of LDS.
hipError_t shared_sample_area_layout(int D, int C, int K, int T, long long num_points, RenderLayout& g) {
    if (T < 1 || T > SAMPLE_AREA_TAPS) return hipErrorInvalidValue;
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    const int P = SSA_TILE / T;
    g.hl = 0;
    g.lds_bytes = sizeof(float) * (((size_t)K + (size_t)SH_KC * SP + 8 + (size_t)(D * D * SSA_AT)
                                    + (size_t)ssa_stage_dwords(C, T, P) + 3) & ~(size_t)3);
    g.workgroups = num_points / P + ((num_points % P != 0) ? 1 : 0);
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    if (g.workgroups > 0x7fffffffLL) return hipErrorNotSupported;
    return hipSuccess;
}

template <int D, int C>
static hipError_t launch_shared_sample_area_dc(const SharedSampleAreaArgs& q, const RenderLayout& g, hipStream_t st) {
    const bool ic = q.s.kc.inverse_cov != 0;
    auto kern = ic ? shared_sample_area_kernel<D, C, true> : shared_sample_area_kernel<D, C, false>;
    return launch_decoder(kern, g.workgroups, SH_THREADS, g.lds_bytes, q, st);
}

// The kernel of a planned call (g from shared_sample_area_layout for the same T = q0.ntaps): the launch alone; it fills ppw,
// the points per workgroup the plan counted with.
hipError_t launch_shared_sample_area(const SharedSampleAreaArgs& q0, int D, int C, const RenderLayout& g, hipStream_t st) {
    if (q0.ntaps < 1 || q0.ntaps > SAMPLE_AREA_TAPS) return hipErrorInvalidValue;
    SharedSampleAreaArgs q = q0;
    q.ppw = SSA_TILE / q.ntaps;
    if (D == 2 && C == 1) return launch_shared_sample_area_dc<2, 1>(q, g, st);
    if (D == 2 && C == 3) return launch_shared_sample_area_dc<2, 3>(q, g, st);
    if (D == 3 && C == 1) return launch_shared_sample_area_dc<3, 1>(q, g, st);
    if (D == 3 && C == 3) return launch_shared_sample_area_dc<3, 3>(q, g, st);
    return hipErrorInvalidValue;
}

}  // namespace smoe
#endif
