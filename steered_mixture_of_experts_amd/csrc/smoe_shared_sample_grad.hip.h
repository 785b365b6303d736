// smoe_shared_sample_grad.hip.h -- analytic spatial derivative of a whole-image (shared-kernel) model at a list of arbitrary
// positions (smoe_shared_sample_grad) or on a dense view given by per-axis tables (smoe_shared_render_view_grad): the Jacobian
// dv_c / dx_l [N, D, C] per source pixel, with the value before the lattice [N, C] and the owning batch [N]
// (include/smoe_hip.h).  Included by smoe_shared.hip after smoe_shared_sample.hip.h; it calls shared_stage_record,
// shared_gate, sample_resolve and render_store_run and changes none.
//
// Definition.  Points, the outside rule, the owning batch and the image-unit coordinate u are smoe_shared_sample's
// (sample_resolve; u = __fdiv_rn(x - 0.5f, (float)(S - 1)), 0 for S == 1); for GRID = true the tables are used with the batch
// index clamped, and nothing is outside.  The evaluated kernels of a point are the compacted list of its batch, exactly as in
// smoe_shared_sample (listed, fake-quantised prior > 0, ascending ids; lists == NULL: every kernel; records from
// shared_stage_record<D, C, IC, false>; the same mode-3 image-wide ranges and centre grid on the host path).  Over them:
//     g_k = shared_gate(...)      S = sum g_k      w_k = g_k * frcp(fmaxf(S, 10e-12f))      M_k = [w_k > tau]
//     e_kc = nu_kc + sum_l Gamma_klc u_l           y_c = sum_k M_k w_k e_kc                  v_c = med3(y_c, 0, nudged_max)
// The gate and y are formed by the same statements in the same order as shared_sample_kernel's sweeps A and B, so
// floorf(fmaf(v_c, inv_scale, 0.5f)) * scale equals smoe_shared_sample's float image bit for bit.
//     s_k = d log g_k / du = -A_k z_k, z_k = A_k^T (u - mu_k)     (train_inverse_cov: s_k = -A_k (u - mu_k), A_k symmetric)
//     sbar = sum_j w_j s_j over ALL evaluated kernels, 0 on the floor of the normaliser (S <= 10e-12)
//     dy_c / du_l = sum_k M_k w_k ((s_kl - sbar_l) e_kc + Gamma_klc)    (the slopes are centred on sbar before they meet the experts)
//     dv = dy where the clip did not act (v_c == y_c), else 0
//     jac[i, l, c] = dv_c / du_l / (S_l - 1) per source pixel, 0 on an axis with S_l == 1
// Mask, clip and lattice are held piecewise constant.  Outside points give 0 / 0 / -1; an inside point whose batch has an
// empty list gives 0 / 0 / its batch id.  A point's three outputs depend on its coordinates, the model and its batch's list
// only: not on N, its place in the list, the other points or the cut of the launch.
//
// The record holds the steering scaled for exp2 (A' = SQ A, or the coefficients SQ^2 A of train_inverse_cov), and the gate
// leaves z' = SQ z: t_kl = (A'_k z'_k)_l = SQ^2 (A_k z_k)_l and s_kl = -t_kl / SQ^2.  1 / SQ^2 = 2 ln 2 is written out
// (SSG_TWO_LN2) and applied once at the end; the square of INV_SQ is 1.7e-5 away from it, which a derivative shows in full.
//     sum_k g_k t_kl is accumulated in sweep A beside S:  tbar_l = frcp(max(S, 1e-11)) sum_k g_k t_kl
//     T_lc = sum_k wt_k (t_kl - tbar_l) e_kc     G_lc = sum_k wt_k Gamma_klc     dy_lc = G_lc - 2 ln 2 T_lc
//
// Arrangement.  shared_sample_kernel's: 256 lanes, lane t the SSG_PPL consecutive points from t * SSG_PPL on, the
// workgroup-uniform walk over the distinct batches of the workgroup's points in ascending id by an LDS atomicMin, the list
// compacted per list word, chunks of SH_KC records, a point's accumulators in registers across the batches.  Two points per
// lane, not four: a point carries S, the D sums of sweep A, y[C], T[D][C] and G[D][C] (30 registers for d = 3, C = 3 beside
// its coordinates) and stages D C + C + 1 dwords, 26 KB for 512 points of d = 3, C = 3 -- DESIGN 3.2h has the compiler's
// figures.  The Jacobians, the values and the batch ids are turned through LDS and leave as one dense run per plane
// (render_store_run): 16-byte non-temporal stores where the plane's base is 16-byte aligned, element-wise at the ragged head
// and tail, 64-bit element offsets.  No inline assembly, no global atomics.
#ifndef SMOE_SHARED_SAMPLE_GRAD_HIP_H
#define SMOE_SHARED_SAMPLE_GRAD_HIP_H

#include "smoe_shared_sample.hip.h"

namespace smoe {

constexpr int SSG_PPL = 2;                               // points per lane
constexpr int SSG_TILE = SH_THREADS * SSG_PPL;           // points per workgroup
constexpr float SSG_TWO_LN2 = 1.3862943611198906f;       // 1 / SQ^2, written out (not INV_SQ * INV_SQ)

// t_l = (A' z')_l from the staged record and the z the gate left: the slope of the log-gate is -2 ln 2 t
template <int D, int C, bool IC>
__device__ __forceinline__ void shared_slope(const float* r, const float (&z)[D], float (&t)[D]) {
    using L = SL<D, C>;
    if (IC) {                                  // z = u - mu; c_ll = A'_ll, c_lm = 2 A'_lm over l > m
#pragma unroll
        for (int l = 0; l < D; ++l) {
            float h = 0.0f;
#pragma unroll
            for (int m = 0; m < D; ++m)
                if (m != l) h = fmaf(r[L::O_AS + ((m < l) ? tri(l, m) : tri(m, l))], z[m], h);
            t[l] = fmaf(0.5f, h, r[L::O_AS + tri(l, l)] * z[l]);
        }
    } else {                                   // z'_m = sum_{l >= m} u_l A'_lm - c_m; t_l = sum_{m <= l} A'_lm z'_m
#pragma unroll
        for (int l = 0; l < D; ++l) {
            float h = 0.0f;
#pragma unroll
            for (int m = 0; m <= l; ++m) h = fmaf(r[L::O_AS + tri(l, m)], z[m], h);
            t[l] = h;
        }
    }
}

template <int D, int C, bool IC, bool GRID>
__global__ void __launch_bounds__(SH_THREADS) shared_sample_grad_kernel(SharedSampleGradArgs q) {
    using L = SL<D, C>;
    const SharedSampleArgs& a = q.s;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int K = a.K;
    const long long p0 = (long long)blockIdx.x * SSG_TILE;             // the workgroup's first point
    const long long pe = (a.num_points - p0 < SSG_TILE) ? a.num_points : p0 + SSG_TILE;

    // LDS carve-up (shared_sample_grad_layout)
    int* s_list = reinterpret_cast<int*>(lds);                       // [K] compacted active kernel ids of the current batch
    float* s_par = lds + K;                                          // [SH_KC][SP]
    int* s_cnt = reinterpret_cast<int*>(s_par + SH_KC * L::SP);      // [8]: 0 list length, 1..4 per wavefront, 5 next batch
    uint32_t* s_jac = reinterpret_cast<uint32_t*>(s_cnt + 8);        // [SSG_TILE][D][C] Jacobian bits
    uint32_t* s_val = s_jac + SSG_TILE * (D * C);                    // [SSG_TILE][C] value bits
    uint32_t* s_bid = s_val + SSG_TILE * C;                          // [SSG_TILE] batch ids

    // ---- 1. this lane's points: image-unit coordinates and owning batch (-1: outside, or past the end of the list) ----
    float x[SSG_PPL][D];
    int bid[SSG_PPL];
#pragma unroll
    for (int j = 0; j < SSG_PPL; ++j) {
        const long long i = p0 + tid * SSG_PPL + j;
        bid[j] = -1;
#pragma unroll
        for (int l = 0; l < D; ++l) x[j][l] = 0.0f;
        if (i >= pe) continue;
        if constexpr (GRID) {
            long long rem = i;
            int idx[D];
#pragma unroll
            for (int l = D - 1; l >= 0; --l) {
                const long long qq = rem / a.ext[l];
                idx[l] = (int)(rem - qq * a.ext[l]);
                rem = qq;
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

    float S[SSG_PPL], inv[SSG_PPL], tb[SSG_PPL][D], y[SSG_PPL][C], T[SSG_PPL][D][C], G[SSG_PPL][D][C];
#pragma unroll
    for (int j = 0; j < SSG_PPL; ++j) {
        S[j] = 0.0f;
        inv[j] = 0.0f;
#pragma unroll
        for (int l = 0; l < D; ++l) tb[j][l] = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            y[j][c] = 0.0f;
#pragma unroll
            for (int l = 0; l < D; ++l) { T[j][l][c] = 0.0f; G[j][l][c] = 0.0f; }
        }
    }

    // ---- 2. the distinct batches of the workgroup's points, ascending (the walk of shared_sample_kernel) ----
    int last = -1;                                                   // the batch just done
    for (;;) {
        int mine = SS_NONE;
#pragma unroll
        for (int j = 0; j < SSG_PPL; ++j)
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

        // ---- 2b. sweep A: gate normaliser, and the gate-weighted slopes beside it ----
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
#pragma unroll
                for (int j = 0; j < SSG_PPL; ++j) {
                    if (bid[j] != cur) continue;
                    float z[D], t[D];
                    const float g = shared_gate<D, C, IC>(r, x[j], z);
                    S[j] += g;
                    shared_slope<D, C, IC>(r, z, t);
#pragma unroll
                    for (int l = 0; l < D; ++l) tb[j][l] = fmaf(g, t[l], tb[j][l]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SSG_PPL; ++j)
            if (bid[j] == cur) {
                inv[j] = frcp(fmaxf(S[j], 10e-12f));
                const bool floor = !(S[j] > 10e-12f);                // the normaliser sits on its floor: a constant, no sbar term
#pragma unroll
                for (int l = 0; l < D; ++l) tb[j][l] = floor ? 0.0f : tb[j][l] * inv[j];
            }

        // ---- 2c. sweep B: masked gate, experts, blend and its derivative ----
        for (int c0 = 0; c0 < Kact; c0 += SH_KC) {
            const int n = min(SH_KC, Kact - c0);
            stage(c0, n);
            for (int kk = 0; kk < n; ++kk) {
                const float* r = s_par + kk * L::SP;
#pragma unroll
                for (int j = 0; j < SSG_PPL; ++j) {
                    if (bid[j] != cur) continue;
                    float z[D], t[D], wd[D];
                    const float w = shared_gate<D, C, IC>(r, x[j], z) * inv[j];
                    const float wt = (w > a.kc.tau) ? w : 0.0f;
                    shared_slope<D, C, IC>(r, z, t);
#pragma unroll
                    for (int l = 0; l < D; ++l) wd[l] = wt * (t[l] - tb[j][l]);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        float ee = r[L::O_NU + c];
#pragma unroll
                        for (int l = 0; l < D; ++l) ee = fmaf(r[L::O_GA + l * C + c], x[j][l], ee);
                        y[j][c] = fmaf(wt, ee, y[j][c]);
#pragma unroll
                        for (int l = 0; l < D; ++l) {
                            T[j][l][c] = fmaf(wd[l], ee, T[j][l][c]);
                            G[j][l][c] = fmaf(wt, r[L::O_GA + l * C + c], G[j][l][c]);
                        }
                    }
                }
            }
        }
        // (the next round begins with a barrier before anything of this batch in LDS is overwritten)
    }

    // ---- 3. clip and its straight-through test, per source pixel; through LDS to the dense planes ----
#pragma unroll
    for (int j = 0; j < SSG_PPL; ++j) {
        const int si = tid * SSG_PPL + j;
        if (p0 + si >= pe) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = __builtin_amdgcn_fmed3f(y[j][c], 0.0f, a.kc.nudged_max);
            s_val[si * C + c] = __float_as_uint((bid[j] >= 0) ? v : 0.0f);
#pragma unroll
            for (int l = 0; l < D; ++l) {
                const float dy = fmaf(-SSG_TWO_LN2, T[j][l][c], G[j][l][c]);
                s_jac[si * (D * C) + l * C + c] = __float_as_uint((bid[j] >= 0 && v == y[j][c]) ? dy * q.du_dx[l] : 0.0f);
            }
        }
        s_bid[si] = (uint32_t)bid[j];
    }
    __syncthreads();
    for (int plane = 0; plane < 3; ++plane) {
        const uint32_t* st = (plane == 0) ? s_jac : ((plane == 1) ? s_val : s_bid);
        void* dst = (plane == 0) ? (void*)q.jac : ((plane == 1) ? (void*)q.values : (void*)q.batch);
        if (dst == nullptr) continue;
        const int cps = (plane == 0) ? D * C : ((plane == 1) ? C : 1);
        const int vs = ((plane == 0) ? q.vec_jac : ((plane == 1) ? q.vec_val : q.vec_bat)) ? 2 : 0;
        const int cpr = ((SSG_TILE * cps + (1 << vs) - 1) >> vs) + 1;            // 16-byte lines the run can touch
        const long long e0 = p0 * cps, e1 = pe * cps;
        for (int ch = tid; ch < cpr; ch += SH_THREADS) render_store_run<false>(st, dst, e0, e1, 0, vs, ch);
    }
}

// The launch geometry and the LDS need of a call for checked arguments: pure host code.  hipErrorNotSupported: 2^31 or more
// workgroups, or more than 160 KB of LDS.
hipError_t shared_sample_grad_layout(int D, int C, int K, long long num_points, RenderLayout& g) {
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    g.hl = 0;
    g.lds_bytes = sizeof(float) * (((size_t)K + (size_t)SH_KC * SP + 8 + (size_t)SSG_TILE * (D * C + C + 1) + 3) & ~(size_t)3);
    g.workgroups = (num_points + SSG_TILE - 1) / SSG_TILE;
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    if (g.workgroups > 0x7fffffffLL) return hipErrorNotSupported;
    return hipSuccess;
}

template <int D, int C>
static hipError_t launch_shared_sample_grad_dc(const SharedSampleGradArgs& q, bool grid, const RenderLayout& g, hipStream_t st) {
    const bool ic = q.s.kc.inverse_cov != 0;
    auto kern = grid ? (ic ? shared_sample_grad_kernel<D, C, true, true> : shared_sample_grad_kernel<D, C, false, true>)
                     : (ic ? shared_sample_grad_kernel<D, C, true, false> : shared_sample_grad_kernel<D, C, false, false>);
    return launch_decoder(kern, g.workgroups, SH_THREADS, g.lds_bytes, q, st);
}

// The kernel of a planned call (g from shared_sample_grad_layout): the launch alone.  grid: the points are the dense view of
// q.s.ext with the per-axis tables q.s.ax / q.s.ab, otherwise the list q.s.points.
hipError_t launch_shared_sample_grad(const SharedSampleGradArgs& q, int D, int C, bool grid, const RenderLayout& g, hipStream_t st) {
    if (D == 2 && C == 1) return launch_shared_sample_grad_dc<2, 1>(q, grid, g, st);
    if (D == 2 && C == 3) return launch_shared_sample_grad_dc<2, 3>(q, grid, g, st);
    if (D == 3 && C == 1) return launch_shared_sample_grad_dc<3, 1>(q, grid, g, st);
    if (D == 3 && C == 3) return launch_shared_sample_grad_dc<3, 3>(q, grid, g, st);
    return hipErrorInvalidValue;
}

}  // namespace smoe
#endif
