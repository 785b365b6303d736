// smoe_sample_area.hip.h -- anti-aliased point decoder: the mean of a fitted block model over a small regular grid of taps
// inside the footprint of every output sample, [N, C] (smoe_sample_area, include/smoe_hip.h).  A decode coarser than the
// source -- a thumbnail, a zoomed-out warp -- takes one position per output cell with smoe_sample and aliases; this one
// integrates over the cell.
//
// Definition.  A point x is the centre of an output cell, in source pixels as for smoe_sample.  The footprint F [d, d]
// (row-major, source pixels) holds in column m the edge vector of the cell along view axis m; taps[m] (1 .. 16, product at most
// 64) is the number of taps along that axis.  One footprint serves all points of a call.  Per point and tap multi-index j, all
// in IEEE fp32:
//     offset     o_m = (float)(2 j_m + 1 - taps[m]) / (float)(2 taps[m])        an exact integer numerator, one rounded division
//     position   t_l = x_l, then for m = 0 .. d-1: t_l = t_l + (F[l][m] * o_m)   product and sum rounded separately, no fma
//     value      the tap is resolved exactly as a point of smoe_sample_grad (outside rule against length, own block g,
//                block-unit coordinate u, with BLEND the same cross-fade) and its value is that call's `values` V, the value
//                before the lattice, bit for bit
//     mean       acc_c = 0, cnt = 0; over the taps in row-major order of j (last axis fastest) an inside tap adds
//                acc_c = acc_c + V_c (one fp32 add) and cnt += 1; mean_c = acc_c / (float)cnt, correctly rounded; cnt == 0: 0.
//                Taps outside the image are left out, not counted as black: an edge cell is as bright as an inside one.
// Outputs: values = the mean put on the lattice by lattice_index (smoe_sample.hip.h), as lattice values or indices; mean; count =
// cnt; block = the own block of the centre, -1 where the centre is outside (its taps inside still give their mean).  No
// argmax: an average has no single kernel.  A point owes nothing to the other points, its place in the list or how the launch
// is cut.  With taps[m] == 1 everywhere the one tap is the point itself: mean is smoe_sample_grad's values.
//
// Arrangement: the point frame of smoe_sample.hip.h with SAMPLE_AREA_PPL points per lane.  The prologue differs from
// point_box in what it bounds: not the blocks of the centres but those of all taps -- per axis the centre's interval
// [x - h, x + h], h = 0.5 sum_m |F[l][m]| (every |o_m| < 0.5), cut to the image, in blocks, widened by one block for the
// roundings of the tap positions (area_box) -- so a centre outside the image with taps inside counts, which point_box would
// drop.  Blend's one block comes on top.  The box's records are staged where they fit the budget (s.rec_cap), otherwise every
// lane derives what it needs (SMOE_SAMPLE_RECORDS applies); a block outside the box (it takes coordinates near 2^24 on blocks
// of one pixel for the roundings to pass a block) is derived directly, so both paths give the same bits whatever the box.
// The products F[l][m] * o_m are made once per workgroup into an LDS table [d][d][16]; a lane walks the taps of its point with
// a run-time trip count and a carried multi-index, adds the d products to each coordinate, and keeps the record of the block
// it evaluated last: taps one source pixel apart mostly share a block.  The evaluation (area_value) is the value half of
// grad_eval -- gate, mask, experts in the same fused multiply-adds in the same order, then the clip and with BLEND the
// cross-fade and the quotient as sample_grad_kernel has them -- and computes no slopes.  The four planes (values, mean,
// count, block) leave after one barrier through point_store_plane.
// One point per lane: the body is not unrolled over a lane's points, so the registers do not depend on the number, and a
// point is up to 64 evaluations -- 256 points already are a workgroup's worth of work, a thumbnail has few points, and the
// fewer consecutive centres a workgroup takes the smaller the box of their footprints.  A point stages 2 C + 2 dwords (values and
// mean apart: the planes are stored from the staging as they are), 8 KB at C = 3 beside at most 12 KB of records: the register
// file sets the occupancy for every triple (DESIGN 3.2i has the figures).
#ifndef SMOE_SAMPLE_AREA_HIP_H
#define SMOE_SAMPLE_AREA_HIP_H

#include "smoe_sample_grad.hip.h"

namespace smoe {

constexpr int SAMPLE_AREA_PPL = 1;                          // points per lane

// One block at block-unit position x: the masked gate wt and the pre-clip blend y -- grad_eval without its slopes, statement
// for statement, so y has grad_eval's bits.
template <int D, int C, int K, bool IC>
__device__ __forceinline__ void area_value(const BlockRegs<D, C, K>& R, const KernelConsts& kc, const float (&x)[D],
                                           float (&wt)[K], float (&y)[C]) {
    float g[K];
    float S = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float maha = 0.0f;
        if (IC) {
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
        } else {
#pragma unroll
            for (int m = 0; m < D; ++m) {
                float zz = -R.cz[k][m];
#pragma unroll
                for (int l = D - 1; l >= m; --l) zz = fmaf(x[l], R.As[k][tri_index(l, m)], zz);
                maha = (m == 0) ? zz * zz : fmaf(zz, zz, maha);
            }
        }
        g[k] = R.coef[k] * fast_exp2(-maha);
        S = (k == 0) ? g[k] : S + g[k];
    }
    const float inv = fast_rcp(fmaxf(S, 10e-12f));
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float w = g[k] * inv;
        wt[k] = (w > kc.tau) ? w : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float ee = R.nu(k, c);
#pragma unroll
            for (int l = 0; l < D; ++l) ee = fmaf(R.ga(k, l, c), x[l], ee);
            y[c] = (k == 0) ? wt[k] * ee : fmaf(wt[k], ee, y[c]);
        }
    }
}

// The prologue up to the box, with two barriers (point_box's, for footprints): the box of the blocks the taps of the
// workgroup's points can lie in.  Per axis a centre x covers [x - h, x + h] cut to [0, length]; its blocks, one more on either
// side, inside the grid.  A centre whose interval misses the image on some axis (a NaN does) has no tap inside and adds nothing.
template <int D, int PPL, bool BLEND>
__device__ __forceinline__ long long area_box(const SampleAreaArgs& q, float* lds, long long p0, long long pe, int (&lo)[D],
                                              int (&nbx)[D]) {
    const SampleArgs& s = q.s;
    const RenderArgs& a = s.r;
    const int tid = threadIdx.x;
    int* s_box = reinterpret_cast<int*>(lds);
    if (tid < D) { s_box[2 * tid] = 0x7fffffff; s_box[2 * tid + 1] = -1; }
    __syncthreads();
    for (int j = 0; j < PPL; ++j) {
        const long long i = p0 + tid * PPL + j;
        if (i >= pe) break;
        float c0[D], c1[D];
        bool any = true;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            const float x = s.points[i * D + l];
            c0[l] = x - q.half[l];
            c1[l] = x + q.half[l];
            any = any && (c1[l] >= 0.0f) && (c0[l] < s.length[l]);
        }
        if (any) {
#pragma unroll
            for (int l = 0; l < D; ++l) {                  // (0 <= the cut interval <= length <= 2^24: the conversions are exact)
                const float fn = (float)s.n[l];
                const int g0 = max((int)floorf(fmaxf(c0[l], 0.0f) / fn) - 1, 0);
                const int g1 = min((int)floorf(fminf(c1[l], s.length[l]) / fn) + 1, a.grid[l] - 1);
                if (g0 < s_box[2 * l]) atomicMin(&s_box[2 * l], g0);
                if (g1 > s_box[2 * l + 1]) atomicMax(&s_box[2 * l + 1], g1);
            }
        }
    }
    __syncthreads();
    long long nrec = 1;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        int b0 = s_box[2 * l], b1 = s_box[2 * l + 1];
        if (BLEND && s.band[l] > 0.0f) { b0 = max(b0 - 1, 0); b1 = min(b1 + 1, a.grid[l] - 1); }
        // (an empty box starts at block 0, not at the minimum's initial value: point_locate_at forms a tap's record index from
        // lo and nbx before the kernel's in-box test discards it, and with lo = 0 and block indices below 2^24 that stays in range)
        lo[l] = (b1 >= b0) ? b0 : 0;
        nbx[l] = (b1 >= b0) ? b1 - b0 + 1 : 0;
        nrec *= nbx[l];
    }
    return nrec;
}

template <int D, int C, int K, bool QUANT, bool IC, bool BLEND>
__global__ void __launch_bounds__(RENDER_THREADS) sample_area_kernel(SampleAreaArgs q) {
    constexpr int per = SAMPLE_AREA_PPL * RENDER_THREADS;
    constexpr int AT = SAMPLE_AREA_AXIS_TAPS;
    const SampleArgs& s = q.s;
    const RenderArgs& a = s.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * per;      // the workgroup's points [p0, pe)
    const long long pe = (s.num_points - p0 < per) ? s.num_points : p0 + per;
    // the tap table: s_tap[(l * D + m) * AT + j] = F[l][m] * o_m(j), 0 past taps[m]; area_box's barriers publish it
    float* s_tap = lds + q.off_tap;
    if (tid < AT) {
#pragma unroll
        for (int m = 0; m < D; ++m) {
            const int nt = q.taps[m];
            const float o = (tid < nt) ? __fdiv_rn((float)(2 * tid + 1 - nt), (float)(2 * nt)) : 0.0f;
#pragma unroll
            for (int l = 0; l < D; ++l) s_tap[(l * D + m) * AT + tid] = __fmul_rn(q.F[l * D + m], o);
        }
    }
    int lo[D], nbx[D];                                     // the box: first block and blocks per axis
    float* s_rec = lds + a.off_par;
    const long long nrec = area_box<D, SAMPLE_AREA_PPL, BLEND>(q, lds, p0, pe, lo, nbx);
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
    // staging: the lattice values, the means, the counts and the block indices of the workgroup's points
    uint32_t* sv = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    uint32_t* sm = sv + per * C;
    uint32_t* sc = sm + per * C;
    uint32_t* sbk = sc + per;
    const int ntaps = q.ntaps;
#pragma unroll 1
    for (int j = 0; j < SAMPLE_AREA_PPL; ++j) {
        const int si = tid * SAMPLE_AREA_PPL + j;
        const long long i = p0 + si;
        if (i < pe) {
            float xc[D], acc[C];
            int jm[D];
#pragma unroll
            for (int l = 0; l < D; ++l) { xc[l] = s.points[i * D + l]; jm[l] = 0; }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.0f;
            int cnt = 0;
#pragma unroll 1
            for (int t = 0; t < ntaps; ++t) {
                float tp[D];
#pragma unroll
                for (int l = 0; l < D; ++l) {
                    float v = xc[l];
#pragma unroll
                    for (int m = 0; m < D; ++m) v = __fadd_rn(v, s_tap[(l * D + m) * AT + jm[m]]);
                    tp[l] = v;
                }
                bool carry = true;                         // the next multi-index, last axis fastest
#pragma unroll
                for (int m = D - 1; m >= 0; --m) {
                    const int nx = jm[m] + 1;
                    const bool wrap = nx >= q.taps[m];
                    jm[m] = carry ? (wrap ? 0 : nx) : jm[m];
                    carry = carry && wrap;
                }
                float x[D];
                int g[D], rec;
                long long id;
                if (point_locate_at<D>(s, lo, nbx, tp, g, x, id, rec)) {
                    if (id != cur_id) {                    // the tap lies in another block: its record
                        bool inbox = true;
#pragma unroll
                        for (int l = 0; l < D; ++l) inbox = inbox && g[l] >= lo[l] && g[l] - lo[l] < nbx[l];
                        point_fetch<D, C, K, QUANT, IC>(s, staged && inbox, s_rec, R, id, rec);
                        cur_id = id;
                    }
                    float wt[K], y[C], v[C];
                    area_value<D, C, K, IC>(R, a.kc, x, wt, y);
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = __builtin_amdgcn_fmed3f(y[c], 0.0f, a.kc.nudged_max);
                    if constexpr (BLEND) {
                        float wn[D];                       // weight of the neighbour per axis, sd: its side
                        int sd[D];
                        bool band = false;
#pragma unroll
                        for (int l = 0; l < D; ++l) {
                            point_window(s, l, x[l], g[l], sd[l], wn[l]);
                            band = band || (wn[l] > 0.0f);
                        }
                        if (band) {
                            float den = 0.0f, num[C];
                            if (has_influence<K>(wt)) {
                                den = 1.0f;
#pragma unroll
                                for (int l = 0; l < D; ++l) den *= 1.0f - wn[l];
                            }
#pragma unroll
                            for (int c = 0; c < C; ++c) num[c] = den * v[c];
#pragma unroll 1
                            for (int cm = 1; cm < (1 << D); ++cm) {
                                float xn[D];
                                int nrc;
                                long long nid;
                                const float Wc = point_corner<D>(s, lo, nbx, cm, g, x, sd, wn, xn, nid, nrc);
                                if (Wc > 0.0f) {
                                    bool inbox = true;
#pragma unroll
                                    for (int l = 0; l < D; ++l) {
                                        const int gg = g[l] + ((((cm >> l) & 1) != 0) ? sd[l] : 0);
                                        inbox = inbox && gg >= lo[l] && gg - lo[l] < nbx[l];
                                    }
                                    BlockRegs<D, C, K> N;
                                    point_fetch<D, C, K, QUANT, IC>(s, staged && inbox, s_rec, N, nid, nrc);
                                    float wtn[K], yn[C];
                                    area_value<D, C, K, IC>(N, a.kc, xn, wtn, yn);
                                    if (has_influence<K>(wtn)) {
                                        den += Wc;
#pragma unroll
                                        for (int c = 0; c < C; ++c)
                                            num[c] = fmaf(Wc, __builtin_amdgcn_fmed3f(yn[c], 0.0f, a.kc.nudged_max), num[c]);
                                    }
                                }
                            }
#pragma unroll
                            for (int c = 0; c < C; ++c) v[c] = (den > 0.0f) ? num[c] / den : 0.0f;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], v[c]);
                    ++cnt;
                }
            }
            // the centre's own block
            long long cid = 0;
            bool cin = true;
#pragma unroll
            for (int l = 0; l < D; ++l) {
                int gc;
                float uc;
                cin = sample_resolve(xc[l], s.n[l], s.length[l], gc, uc) && cin;
                cid = cid * a.grid[l] + gc;
            }
            // the point into the staging buffers: its mean, the mean on the lattice in the output's format, its count, its block
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float mean = (cnt > 0) ? __fdiv_rn(acc[c], (float)cnt) : 0.0f;
                const float kq = lattice_index(a.kc, mean);
                sm[si * C + c] = __float_as_uint(mean);
                sv[si * C + c] = (a.fmt == SMOE_IMAGE_U8) ? (uint32_t)kq : __float_as_uint(kq * a.kc.scale);
            }
            sc[si] = (uint32_t)cnt;
            sbk[si] = (uint32_t)(int)(cin ? cid : -1);
        }
    }
    __syncthreads();
    if (a.image != nullptr) {
        const bool u8 = a.fmt == SMOE_IMAGE_U8;
        point_store_plane<SAMPLE_AREA_PPL>(p0, pe, sv, a.image, C, a.vec_img ? (u8 ? 4 : 2) : 0, u8);
    }
    if (q.mean != nullptr) point_store_plane<SAMPLE_AREA_PPL>(p0, pe, sm, q.mean, C, q.vec_mean ? 2 : 0, false);
    if (q.count != nullptr) point_store_plane<SAMPLE_AREA_PPL>(p0, pe, sc, q.count, 1, q.vec_cnt ? 4 : 0, true);
    if (s.block != nullptr) point_store_plane<SAMPLE_AREA_PPL>(p0, pe, sbk, s.block, 1, s.vec_blk ? 2 : 0, false);
}

// The launch geometry and the LDS carve-up for checked arguments (point_layout): a point stages its lattice values, its mean,
// its count and its block; the tap table follows the staging; there is no hoisting level.
template <int D, int C, int K, bool FULL>
hipError_t sample_area_layout(SampleAreaArgs& q, long long records, RenderLayout& g) {
    if (q.s.r.kc.qmode != 0 && !FULL) return hipErrorNotSupported;
    g.hl = 0;
    const hipError_t e = point_layout(D, 2 * C + 2, SAMPLE_AREA_PPL, BlendRec<D, C, K>::STRIDE, records, q.s, g);
    if (e != hipSuccess) return e;
    q.off_tap = round_up(q.s.r.off_stage + SAMPLE_AREA_PPL * RENDER_THREADS * (2 * C + 2), 4);
    g.lds_bytes = sizeof(float) * ((size_t)q.off_tap + (size_t)(D * D * SAMPLE_AREA_AXIS_TAPS));
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    return hipSuccess;
}

// the instantiation for (fake-quantised graph, inverse covariance); the fake-quantised ones exist for FULL triples
template <int D, int C, int K, bool FULL, bool BLEND>
auto sample_area_kernel_for(bool quant, bool ic) -> void (*)(SampleAreaArgs) {
    if constexpr (FULL) {
        if (quant) return ic ? &sample_area_kernel<D, C, K, true, true, BLEND> : &sample_area_kernel<D, C, K, true, false, BLEND>;
    }
    if (quant) return nullptr;
    return ic ? &sample_area_kernel<D, C, K, false, true, BLEND> : &sample_area_kernel<D, C, K, false, false, BLEND>;
}

// The kernel of a planned call (geometry filled by sample_area_layout): the launch alone.
template <int D, int C, int K, bool FULL>
hipError_t launch_sample_area(const SampleAreaArgs& q, const RenderLayout& g, hipStream_t st) {
    const bool quant = q.s.r.kc.qmode != 0;
    bool blend = false;
    for (int l = 0; l < D; ++l) blend = blend || q.s.band[l] > 0.0f;
    const auto kern = blend ? sample_area_kernel_for<D, C, K, FULL, true>(quant, q.s.r.kc.inverse_cov != 0)
                            : sample_area_kernel_for<D, C, K, FULL, false>(quant, q.s.r.kc.inverse_cov != 0);
    if (kern == nullptr) return hipErrorNotSupported;
    return launch_decoder(kern, g.workgroups, RENDER_THREADS, g.lds_bytes, q, st);
}

}  // namespace smoe
#endif
