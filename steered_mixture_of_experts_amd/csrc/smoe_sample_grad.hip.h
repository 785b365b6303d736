// smoe_sample_grad.hip.h -- analytic spatial derivative of a fitted block model at a list of arbitrary positions: the
// Jacobian dV_c / dx_l [N, D, C] per source pixel, with the value before the lattice [N, C] and the own block [N]
// (smoe_sample_grad, include/smoe_hip.h).
//
// Definition.  Points, outside rule, own block g and block-unit coordinate u are smoe_sample's (sample_resolve); the model
// state of a block is what sample_derive leaves (fake quantisation, centre grid, train_gammas, only_y_gamma, inverse
// covariance).  One block at u, over its evaluated kernels (listed, pis > 0):
//     g_k = coef_k exp(-m_k / 2)    S = sum g_k    w_k = g_k / max(S, 1e-11)    M_k = [w_k > tau]
//     e_kc = nu_kc + sum_l Gamma_klc u_l           y_c = sum_k M_k w_k e_kc      v_c = clip(y_c, 0, nudged_max)
//     s_k = d log g_k / du = -A_k z_k, z_k = A_k^T (u - mu_k)      (train_inverse_cov: s_k = -A_k (u - mu_k), A_k symmetric)
//     sbar = sum_j w_j s_j over all evaluated kernels where S > 1e-11, 0 on the floor (the normaliser is a constant there)
//     dy_c / du_l = sum_k M_k w_k ((s_kl - sbar_l) e_kc + Gamma_klc)           (the mask is piecewise constant)
//     dv_c / du_l = dy_c / du_l where clip(y_c) == y_c, else 0                  (the fit kernel's straight-through test)
// The 8-bit lattice is ignored: this is the derivative of the value before floor(v (2^p - 1) + 1/2).
// Blend: windows, neighbour coordinates u -+ n / (n - 1), zero weight outside the grid and the drop of blocks without
// influence are smoe_render_blend's.  d|w_l| / du_l = +0.5 / b_l for the high neighbour and -0.5 / b_l for the low one where
// the ratio lies strictly inside (0, 1), 0 where it is clamped or the neighbour is outside the grid; W_b is the product over
// the axes of |w_l| or 1 - |w_l| and dW_b follows by the product rule; over the blocks kept
//     V = sum W_b v_b / sum W_b        dV = (sum (dW_b v_b + W_b dv_b) - V sum dW_b) / sum W_b
// (a neighbour's coordinate is u plus a constant: no chain factor); no block left: V = 0, dV = 0.
// Units: jac[i, l, c] = dV_c / du_l / (n_l - 1), per source pixel; 0 on an axis with n_l == 1.  Outside points: jac 0, values
// 0, block -1.  A point owes nothing to the other points, to its place in the list or to how the launch is cut.
//
// Arrangement: the point frame of smoe_sample.hip.h (the workgroup's points and box, the staged / direct record
// paths, locating a point, the neighbour windows and corners, the plane stores) with SAMPLE_GRAD_PPL points per lane; the
// evaluation, the slopes of the windows and the quotient rule are this kernel's.  There is no hoisting level: every point has
// its own coordinate on every axis, and the forward half of grad_eval is pixel<>'s order of operations without hoisting.
// The three planes (Jacobians, values, blocks) are float32 / int32 dwords.
// Two points per lane, not sample_kernel's four: a point stages D C + C + 1 dwords (13 for d = 3, C = 3), so 512 points
// take 26 KB beside at most 12 KB of records and four workgroups fit a CU's 160 KB -- the register file, not LDS, sets the
// occupancy for every triple (DESIGN 3.2g has the figures).  A lane writes its point's D C values at a stride of
// 2 D C dwords from its neighbour's: an even stride, so ds_write_b32 pays a 2-way bank conflict (the 32-bank modulus of
// writes) on 13 dwords per point, against several hundred VALU instructions for the same point.
#ifndef SMOE_SAMPLE_GRAD_HIP_H
#define SMOE_SAMPLE_GRAD_HIP_H

#include "smoe_sample.hip.h"

namespace smoe {

constexpr int SAMPLE_GRAD_PPL = 2;                          // points per lane
// 1 / SQ^2 = 2 ln 2, written out: the square of SMOE_INV_SQ is 1.7e-5 away from it, which a derivative shows in full
constexpr float SAMPLE_GRAD_INV_SQ2 = 1.3862943611198906f;

// One block at block-unit position x: the masked gate wt, the pre-clip blend y and its derivative dy[l][c] = dy_c / du_l.
// The gate, the experts and y are formed as pixel<> forms them without hoisting (the same fused multiply-adds in the same
// order).  t_kl = (A'_k z'_k)_l = SQ^2 (A_k z_k)_l, so s_kl = -t_kl / SQ^2; the factor is applied once at the end:
//     dy_lc = G_lc - T_lc / SQ^2,   T_lc = sum_k wt_k (t_kl - tbar_l) e_kc,  tbar_l = sum_k w_k t_kl,  G_lc = sum_k wt_k Gamma_klc
template <int D, int C, int K, bool IC>
__device__ __forceinline__ void grad_eval(const BlockRegs<D, C, K>& R, const KernelConsts& kc, const float (&x)[D],
                                          float (&wt)[K], float (&y)[C], float (&dy)[D][C]) {
    float g[K], t[K][D];
    float S = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float maha = 0.0f;
        if (IC) {
            // maha' = r^T A' r over the packed quadratic form (c_ll = A'_ll, c_lm = 2 A'_lm); (A' r)_l from the same coefficients
            float r[D];
#pragma unroll
            for (int l = 0; l < D; ++l) r[l] = x[l] - R.mu(k, l);
#pragma unroll
            for (int l = 0; l < D; ++l) {
                float tq = 0.0f;
#pragma unroll
                for (int m = 0; m <= l; ++m) tq = fmaf(R.As[k][tri_index(l, m)], r[m], tq);
                maha = fmaf(tq, r[l], maha);
            }
#pragma unroll
            for (int l = 0; l < D; ++l) {
                float h = 0.0f;
#pragma unroll
                for (int m = 0; m < D; ++m)
                    if (m != l) h = fmaf(R.As[k][(m < l) ? tri_index(l, m) : tri_index(m, l)], r[m], h);
                t[k][l] = fmaf(0.5f, h, R.As[k][tri_index(l, l)] * r[l]);
            }
        } else {
#pragma unroll
            for (int m = 0; m < D; ++m) {
                float zz = -R.cz[k][m];
#pragma unroll
                for (int l = D - 1; l >= m; --l) zz = fmaf(x[l], R.As[k][tri_index(l, m)], zz);
                maha = (m == 0) ? zz * zz : fmaf(zz, zz, maha);
            }
            // the slope from r = x - mu rather than from the gate's z' = x A' - c (a difference of two products): one rounding
            // less in front of the multiplication by A'
            float r[D], zr[D];
#pragma unroll
            for (int l = 0; l < D; ++l) r[l] = x[l] - R.mu(k, l);
#pragma unroll
            for (int m = 0; m < D; ++m) {
                float zz = 0.0f;
#pragma unroll
                for (int l = D - 1; l >= m; --l) zz = fmaf(r[l], R.As[k][tri_index(l, m)], zz);
                zr[m] = zz;
            }
#pragma unroll
            for (int l = 0; l < D; ++l) {
                float h = 0.0f;
#pragma unroll
                for (int m = 0; m <= l; ++m) h = fmaf(R.As[k][tri_index(l, m)], zr[m], h);
                t[k][l] = h;
            }
        }
        g[k] = R.coef[k] * fast_exp2(-maha);
        S = (k == 0) ? g[k] : S + g[k];
    }
    const float inv = fast_rcp(fmaxf(S, 10e-12f));
    float w[K], tb[D], T[D][C], G[D][C];
#pragma unroll
    for (int l = 0; l < D; ++l) {
        tb[l] = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) { T[l][c] = 0.0f; G[l][c] = 0.0f; }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = g[k] * inv;
        wt[k] = (w[k] > kc.tau) ? w[k] : 0.0f;
#pragma unroll
        for (int l = 0; l < D; ++l) tb[l] = fmaf(w[k], t[k][l], tb[l]);
    }
    if (!(S > 10e-12f)) {                                  // the normaliser sits on its floor: a constant, no sbar term
#pragma unroll
        for (int l = 0; l < D; ++l) tb[l] = 0.0f;
    } else if (K == 1) {
        // one kernel: w = 1 and the mean of the slopes is the one slope, so t - tbar vanishes identically.  w = g * rcp(g) is
        // 1 only to an ulp, and the residue t (1 - w) e would stand in dy beside Gamma at 1e-5 of its size (the same residue
        // the fit kernel removes from its K = 1 gradients)
#pragma unroll
        for (int l = 0; l < D; ++l) tb[l] = t[0][l];
    }
    // the slopes are centred on their mean before they meet the experts, as the definition states them
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float wd[D];
#pragma unroll
        for (int l = 0; l < D; ++l) wd[l] = wt[k] * (t[k][l] - tb[l]);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float ee = R.nu(k, c);
#pragma unroll
            for (int l = 0; l < D; ++l) ee = fmaf(R.ga(k, l, c), x[l], ee);
            y[c] = (k == 0) ? wt[k] * ee : fmaf(wt[k], ee, y[c]);
#pragma unroll
            for (int l = 0; l < D; ++l) {
                T[l][c] = fmaf(wd[l], ee, T[l][c]);
                G[l][c] = fmaf(wt[k], R.ga(k, l, c), G[l][c]);
            }
        }
    }
#pragma unroll
    for (int l = 0; l < D; ++l)
#pragma unroll
        for (int c = 0; c < C; ++c) dy[l][c] = fmaf(-SAMPLE_GRAD_INV_SQ2, T[l][c], G[l][c]);
}

// clip and its straight-through test: v = clip(y), dv = dy where the clip did not act
template <int D, int C>
__device__ __forceinline__ void grad_clip(const KernelConsts& kc, const float (&y)[C], float (&v)[C], float (&dv)[D][C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        v[c] = __builtin_amdgcn_fmed3f(y[c], 0.0f, kc.nudged_max);
#pragma unroll
        for (int l = 0; l < D; ++l) dv[l][c] = (v[c] == y[c]) ? dv[l][c] : 0.0f;
    }
}

template <int D, int C, int K, bool QUANT, bool IC, bool BLEND>
__global__ void __launch_bounds__(RENDER_THREADS) sample_grad_kernel(SampleGradArgs q) {
    constexpr int per = SAMPLE_GRAD_PPL * RENDER_THREADS;
    const SampleArgs& s = q.s;
    const RenderArgs& a = s.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * per;      // the workgroup's points [p0, pe)
    const long long pe = (s.num_points - p0 < per) ? s.num_points : p0 + per;
    int lo[D], nbx[D];                                     // the box: first block and blocks per axis
    float* s_rec = lds + a.off_par;
    const long long nrec = point_box<D, SAMPLE_GRAD_PPL, BLEND>(s, lds, p0, pe, lo, nbx);
    const bool staged = nrec <= (long long)s.rec_cap;      // workgroup-uniform
    if (staged) {
        for (int rec = tid; rec < (int)nrec; rec += RENDER_THREADS) {
            long long id = 0;
            int r = rec, sl[D];
#pragma unroll
            for (int l = D - 1; l >= 0; --l) {
                const int rr = r / nbx[l];
                sl[l] = r - rr * nbx[l];
                r = rr;
            }
#pragma unroll
            for (int l = 0; l < D; ++l) id = id * a.grid[l] + (lo[l] + sl[l]);
            BlockRegs<D, C, K> B;
            sample_derive<D, C, K, QUANT, IC>(a, id, B);
            store_record<D, C, K>(B, s_rec + rec * BlendRec<D, C, K>::STRIDE);
        }
    }
    __syncthreads();

    BlockRegs<D, C, K> R;
    long long cur_id = -1;
    // staging: the Jacobians, the values and the block indices of the workgroup's points
    uint32_t* sj = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    uint32_t* sv = sj + per * (D * C);
    uint32_t* sbk = sv + per * C;
#pragma unroll 1
    for (int j = 0; j < SAMPLE_GRAD_PPL; ++j) {
        const int si = tid * SAMPLE_GRAD_PPL + j;          // the lane's points are neighbours: mostly one block, one record
        const long long i = p0 + si;
        if (i < pe) {
            float x[D];
            int g[D], rec;
            long long id;
            float v[C], dv[D][C];
            if (point_locate<D>(s, lo, nbx, i, g, x, id, rec)) {
                if (id != cur_id) {                        // the point lies in another block: its record
                    point_fetch<D, C, K, QUANT, IC>(s, staged, s_rec, R, id, rec);
                    cur_id = id;
                }
                float wt[K], y[C];
                grad_eval<D, C, K, IC>(R, a.kc, x, wt, y, dv);
                grad_clip<D, C>(a.kc, y, v, dv);
                if constexpr (BLEND) {
                    float wn[D], dwn[D];                   // weight of the neighbour per axis and its slope, sd: its side
                    int sd[D];
                    bool band = false;
#pragma unroll
                    for (int l = 0; l < D; ++l) {
                        const float w = point_window(s, l, x[l], g[l], sd[l], wn[l]);
                        // strictly inside (0, 1) and the neighbour inside the grid: +-0.5 / b; clamped or outside: 0
                        dwn[l] = (wn[l] > 0.0f && wn[l] < 1.0f) ? ((w > 0.0f) ? 0.5f : -0.5f) / s.band[l] : 0.0f;
                        band = band || (wn[l] > 0.0f);
                    }
                    if (band) {
                        const bool keep = has_influence<K>(wt);
                        float den = 0.0f, dden[D], num[C], dnum[D][C];
#pragma unroll
                        for (int l = 0; l < D; ++l) dden[l] = 0.0f;
                        if (keep) {
                            den = 1.0f;
#pragma unroll
                            for (int l = 0; l < D; ++l) den *= 1.0f - wn[l];
#pragma unroll
                            for (int l = 0; l < D; ++l) {
                                float dW = -dwn[l];
#pragma unroll
                                for (int m = 0; m < D; ++m)
                                    if (m != l) dW *= 1.0f - wn[m];
                                dden[l] = dW;
                            }
                        }
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            num[c] = den * v[c];
#pragma unroll
                            for (int l = 0; l < D; ++l) dnum[l][c] = fmaf(dden[l], v[c], den * dv[l][c]);
                        }
#pragma unroll 1
                        for (int cm = 1; cm < (1 << D); ++cm) {
                            float xn[D], dWc[D];
                            int nrc;
                            long long nid;
                            const float Wc = point_corner<D>(s, lo, nbx, cm, g, x, sd, wn, xn, nid, nrc);
#pragma unroll
                            for (int l = 0; l < D; ++l) {      // the product rule
                                float dW = (((cm >> l) & 1) != 0) ? dwn[l] : -dwn[l];
#pragma unroll
                                for (int m = 0; m < D; ++m)
                                    if (m != l) dW *= (((cm >> m) & 1) != 0) ? wn[m] : 1.0f - wn[m];
                                dWc[l] = dW;
                            }
                            if (Wc > 0.0f) {               // (weight 0: its slopes are 0 too)
                                BlockRegs<D, C, K> N;
                                point_fetch<D, C, K, QUANT, IC>(s, staged, s_rec, N, nid, nrc);
                                float wtn[K], yn[C], vn[C], dvn[D][C];
                                grad_eval<D, C, K, IC>(N, a.kc, xn, wtn, yn, dvn);
                                if (has_influence<K>(wtn)) {
                                    grad_clip<D, C>(a.kc, yn, vn, dvn);
                                    den += Wc;
#pragma unroll
                                    for (int l = 0; l < D; ++l) dden[l] += dWc[l];
#pragma unroll
                                    for (int c = 0; c < C; ++c) {
                                        num[c] = fmaf(Wc, vn[c], num[c]);
#pragma unroll
                                        for (int l = 0; l < D; ++l) dnum[l][c] = fmaf(dWc[l], vn[c], fmaf(Wc, dvn[l][c], dnum[l][c]));
                                    }
                                }
                            }
                        }
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            v[c] = (den > 0.0f) ? num[c] / den : 0.0f;
#pragma unroll
                            for (int l = 0; l < D; ++l) dv[l][c] = (den > 0.0f) ? fmaf(-v[c], dden[l], dnum[l][c]) / den : 0.0f;
                        }
                    }
                }
#pragma unroll
                for (int l = 0; l < D; ++l)
#pragma unroll
                    for (int c = 0; c < C; ++c) dv[l][c] *= q.du_dx[l];      // per source pixel
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    v[c] = 0.0f;
#pragma unroll
                    for (int l = 0; l < D; ++l) dv[l][c] = 0.0f;
                }
            }
            // the point into the staging buffers: its Jacobian [D][C], its values, its block
#pragma unroll
            for (int l = 0; l < D; ++l)
#pragma unroll
                for (int c = 0; c < C; ++c) sj[si * (D * C) + l * C + c] = __float_as_uint(dv[l][c]);
#pragma unroll
            for (int c = 0; c < C; ++c) sv[si * C + c] = __float_as_uint(v[c]);
            sbk[si] = (uint32_t)(int)id;
        }
    }
    __syncthreads();
    point_store_plane<SAMPLE_GRAD_PPL>(p0, pe, sj, q.jac, D * C, q.vec_jac ? 2 : 0, false);
    if (q.values != nullptr) point_store_plane<SAMPLE_GRAD_PPL>(p0, pe, sv, q.values, C, q.vec_val ? 2 : 0, false);
    if (s.block != nullptr) point_store_plane<SAMPLE_GRAD_PPL>(p0, pe, sbk, s.block, 1, s.vec_blk ? 2 : 0, false);
}

// The launch geometry and the LDS carve-up for checked arguments (point_layout): a point stages its Jacobian, its values and
// its block; there is no hoisting level.
template <int D, int C, int K, bool FULL>
hipError_t sample_grad_layout(SampleGradArgs& q, long long records, RenderLayout& g) {
    if (q.s.r.kc.qmode != 0 && !FULL) return hipErrorNotSupported;
    g.hl = 0;
    return point_layout(D, D * C + C + 1, SAMPLE_GRAD_PPL, BlendRec<D, C, K>::STRIDE, records, q.s, g);
}

// the instantiation for (fake-quantised graph, inverse covariance); the fake-quantised ones exist for FULL triples
template <int D, int C, int K, bool FULL, bool BLEND>
auto sample_grad_kernel_for(bool quant, bool ic) -> void (*)(SampleGradArgs) {
    if constexpr (FULL) {
        if (quant) return ic ? &sample_grad_kernel<D, C, K, true, true, BLEND> : &sample_grad_kernel<D, C, K, true, false, BLEND>;
    }
    if (quant) return nullptr;
    // WITHHELD: <3, 3, 6, QUANT = false, IC = false, BLEND = true>.  On the MI355X this one instantiation (386 registers, no
    // scratch) returned block ids and values that depend on the other points of the list, and on the direct record path an
    // illegal address; the source is the one every other triple runs, and the cause is open.  It is not built; smoe_sample_grad
    // refuses the call by name (csrc/smoe_capi.hip), and this is the same answer for any other caller.
    if constexpr (D == 3 && C == 3 && K == 6 && BLEND) {
        return ic ? &sample_grad_kernel<D, C, K, false, true, BLEND> : nullptr;
    } else {
        return ic ? &sample_grad_kernel<D, C, K, false, true, BLEND> : &sample_grad_kernel<D, C, K, false, false, BLEND>;
    }
}

// The kernel of a planned call (geometry filled by sample_grad_layout): the launch alone.
template <int D, int C, int K, bool FULL>
hipError_t launch_sample_grad(const SampleGradArgs& q, const RenderLayout& g, hipStream_t st) {
    const bool quant = q.s.r.kc.qmode != 0;
    bool blend = false;
    for (int l = 0; l < D; ++l) blend = blend || q.s.band[l] > 0.0f;
    const auto kern = blend ? sample_grad_kernel_for<D, C, K, FULL, true>(quant, q.s.r.kc.inverse_cov != 0)
                            : sample_grad_kernel_for<D, C, K, FULL, false>(quant, q.s.r.kc.inverse_cov != 0);
    if (kern == nullptr) return hipErrorNotSupported;
    return launch_decoder(kern, g.workgroups, RENDER_THREADS, g.lds_bytes, q, st);
}

}  // namespace smoe
#endif
