// smoe_sample_area_each.hip.h -- anti-aliased point decoder with a footprint and tap counts of its own for every point
// (smoe_sample_area_each, include/smoe_hip.h): smoe_sample_area for views whose magnification varies across the output -- a
// perspective view, a lens map, any dense lookup map.
//
// Definition.  Point i has the centre x = points[i], the footprint F = footprints[i] ([d, d] row-major, source pixels) and the
// tap counts n = taps[i] (a byte per view axis).  Its result is that of smoe_sample_area (smoe_sample_area.hip.h) called with
// this one point, this footprint and these taps, bit for bit: per tap multi-index j, all in IEEE fp32,
//     offset     o_m = (float)(2 j_m + 1 - n_m) / (float)(2 n_m)
//     position   t_l = x_l, then for m = 0 .. d-1: t_l = t_l + (F[l][m] * o_m)      product and sum rounded separately
//     value, mean, outputs: word for word as there (row-major order of j, inside taps only, one division, lattice_index).
// A point is VOID if a tap count is outside 1 .. 16, if their product is above 64 or if an entry of its footprint is not finite:
// values 0, mean 0, count 0, block = the centre's own block as for every point.  The host cannot read the device arrays, so
// this is a defined result and not an error; a void point takes no tap (its trip count is 0, every other point's at most 64,
// whatever bytes the arrays hold) and reads the offset table at row 1 only.  A point owes nothing to the other points, its
// place in the list or how the launch is cut.
//
// Arrangement: sample_area_kernel's, with four differences.
//  * Tap offsets.  No table of products: the workgroup builds the offsets alone, s_tab[(n - 1) * 16 + j] = o(n, j) for n in
//    1 .. 16 and j < n (0 past n), one __fdiv_rn per entry and lane, 1 KB; a lane forms __fmul_rn(F[l][m], o) per tap -- the
//    same two operands sample_area_kernel's table multiplies, so the same bits.
//  * Footprints and tap counts.  The workgroup's run of both arrays is contiguous: it is copied into LDS once (area_each_stage:
//    16-byte / 4-byte loads where the array's base is aligned so and the line lies inside the run, element-wise otherwise -- a
//    copy, so the same bits either way) and a lane reads its own slot, stride d * d dwords (odd: no bank conflicts).  A lane
//    re-reads its F from the slot for every tap, through an address the compiler cannot see through, so that the d * d values
//    are not carried in registers across the evaluation (SAMPLE_AREA_EACH_F_REGS = 1 keeps them in registers: 8 .. 10 more
//    VGPRs and a wave per SIMD less on the cross-fades of d = 3, C = 3; DESIGN 3.2k has the figures of both choices).
//  * The box.  Per point h_l = 0.5 sum_m |F[l][m]| in fp32, a shade widened; not rounded up exactly and it need not be: a
//    tap whose block falls outside the box is derived directly and gives the same bits (smoe_sample_area.hip.h), so the box
//    is a performance device only.  A void point adds nothing to it.  One point with a huge footprint (near a horizon |F|
//    reaches thousands of pixels) makes the box the whole image and sends its workgroup onto the direct path.
//  * Divergence.  The trip count is the lane's own; neighbouring samples of a smooth view have similar footprints.  Points are
//    not sorted or re-binned.
#ifndef SMOE_SAMPLE_AREA_EACH_HIP_H
#define SMOE_SAMPLE_AREA_EACH_HIP_H

#include "smoe_sample_area.hip.h"

namespace smoe {

#ifndef SAMPLE_AREA_EACH_F_REGS
#define SAMPLE_AREA_EACH_F_REGS 0                           // a lane's footprint: 1 in registers, 0 re-read from its LDS slot per tap
#endif

static_assert(RENDER_THREADS == SAMPLE_AREA_AXIS_TAPS * SAMPLE_AREA_AXIS_TAPS, "one lane per entry of the offset table");

// The workgroup's runs of footprints (floats [f0, f1)) and tap counts (bytes [b0, b1)) into LDS, element k of a run at
// s_fp[k] / s_tp[k].  Nothing outside the runs is read.  The caller's next barrier publishes them.
__device__ __forceinline__ void area_each_stage(const SampleAreaEachArgs& q, long long f0, long long f1, long long b0, long long b1,
                                                float* s_fp, uint8_t* s_tp) {
    const int tid = threadIdx.x;
    if (q.vec_fp) {
        for (long long c = (f0 & ~3LL) + 4LL * tid; c < f1; c += 4LL * RENDER_THREADS) {
            if (c >= f0 && c + 4 <= f1) {
                const float4 v = *reinterpret_cast<const float4*>(q.footprints + c);
                float* d = s_fp + (c - f0);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (c + k >= f0 && c + k < f1) s_fp[c + k - f0] = q.footprints[c + k];
            }
        }
    } else {
        for (long long c = f0 + tid; c < f1; c += RENDER_THREADS) s_fp[c - f0] = q.footprints[c];
    }
    if (q.vec_tap) {
        for (long long c = (b0 & ~3LL) + 4LL * tid; c < b1; c += 4LL * RENDER_THREADS) {
            if (c >= b0 && c + 4 <= b1) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(q.taps + c);
                uint8_t* d = s_tp + (c - b0);
                d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (c + k >= b0 && c + k < b1) s_tp[c + k - b0] = q.taps[c + k];
            }
        }
    } else {
        for (long long c = b0 + tid; c < b1; c += RENDER_THREADS) s_tp[c - b0] = q.taps[c];
    }
}

// area_box for per-point extents: `any` says that the lane's point has taps and that its interval [c0, c1] meets the image on
// every axis.  The kernel has reset the box and passed a barrier (which also published its tables); one more barrier here.
template <int D, bool BLEND>
__device__ __forceinline__ long long area_each_box(const SampleArgs& s, float* lds, bool any, const float (&c0)[D],
                                                   const float (&c1)[D], int (&lo)[D], int (&nbx)[D]) {
    const RenderArgs& a = s.r;
    int* s_box = reinterpret_cast<int*>(lds);
    if (any) {
#pragma unroll
        for (int l = 0; l < D; ++l) {                      // (0 <= the cut interval <= length <= 2^24: the conversions are exact)
            const float fn = (float)s.n[l];
            const int g0 = max((int)floorf(fmaxf(c0[l], 0.0f) / fn) - 1, 0);
            const int g1 = min((int)floorf(fminf(c1[l], s.length[l]) / fn) + 1, a.grid[l] - 1);
            if (g0 < s_box[2 * l]) atomicMin(&s_box[2 * l], g0);
            if (g1 > s_box[2 * l + 1]) atomicMax(&s_box[2 * l + 1], g1);
        }
    }
    __syncthreads();
    long long nrec = 1;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        int b0 = s_box[2 * l], b1 = s_box[2 * l + 1];
        if (BLEND && s.band[l] > 0.0f) { b0 = max(b0 - 1, 0); b1 = min(b1 + 1, a.grid[l] - 1); }
        lo[l] = (b1 >= b0) ? b0 : 0;                       // (an empty box starts at block 0: see area_box)
        nbx[l] = (b1 >= b0) ? b1 - b0 + 1 : 0;
        nrec *= nbx[l];
    }
    return nrec;
}

template <int D, int C, int K, bool QUANT, bool IC, bool BLEND>
__global__ void __launch_bounds__(RENDER_THREADS) sample_area_each_kernel(SampleAreaEachArgs q) {
    constexpr int per = RENDER_THREADS;                     // one point per lane
    constexpr int AT = SAMPLE_AREA_AXIS_TAPS;
    const SampleArgs& s = q.s;
    const RenderArgs& a = s.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * per;      // the workgroup's points [p0, pe)
    const long long pe = (s.num_points - p0 < per) ? s.num_points : p0 + per;
    const long long i = p0 + tid;                          // the lane's point
    // the offset table, the workgroup's footprints and tap counts; the box's first barrier publishes them
    float* s_tab = lds + q.off_tab;
    float* s_fp = lds + q.off_fp;
    uint8_t* s_tp = reinterpret_cast<uint8_t*>(lds + q.off_tap);
    {
        const int n = (tid >> 4) + 1, j = tid & (AT - 1);
        s_tab[tid] = (j < n) ? __fdiv_rn((float)(2 * j + 1 - n), (float)(2 * n)) : 0.0f;
    }
    area_each_stage(q, p0 * (D * D), pe * (D * D), p0 * D, pe * D, s_fp, s_tp);
    int* s_box = reinterpret_cast<int*>(lds);
    if (tid < D) { s_box[2 * tid] = 0x7fffffff; s_box[2 * tid + 1] = -1; }
    __syncthreads();

    // the lane's point: centre, footprint, tap counts; void or past the list: no taps
    float xc[D];
    int nt[D];
    int ntaps = 0;
    const float* Fs = s_fp + tid * (D * D);
#if SAMPLE_AREA_EACH_F_REGS
    float F[D * D];
#endif
    float c0[D], c1[D];
    bool any = false;
#pragma unroll
    for (int l = 0; l < D; ++l) { xc[l] = 0.0f; nt[l] = 1; c0[l] = 0.0f; c1[l] = 0.0f; }
    if (i < pe) {
        bool ok = true;
        int prod = 1;
#pragma unroll
        for (int m = 0; m < D; ++m) {
            const int n = s_tp[tid * D + m];
            ok = ok && n >= 1 && n <= AT;
            prod *= ok ? n : 1;
            nt[m] = n;
        }
        ok = ok && prod <= SAMPLE_AREA_TAPS;
        float h[D];
#pragma unroll
        for (int l = 0; l < D; ++l) {
            xc[l] = s.points[i * D + l];
            float sum = 0.0f;
#pragma unroll
            for (int m = 0; m < D; ++m) {
                const float f = Fs[l * D + m];
#if SAMPLE_AREA_EACH_F_REGS
                F[l * D + m] = f;
#endif
                ok = ok && (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u;
                sum += fabsf(f);
            }
            h[l] = 0.5f * sum * 1.000001f;
        }
        ntaps = ok ? min(prod, SAMPLE_AREA_TAPS) : 0;
        any = ok;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            nt[l] = ok ? nt[l] : 1;
            c0[l] = xc[l] - h[l];
            c1[l] = xc[l] + h[l];
            any = any && (c1[l] >= 0.0f) && (c0[l] < s.length[l]);
        }
    }
#if SAMPLE_AREA_EACH_F_REGS
    else {
#pragma unroll
        for (int e = 0; e < D * D; ++e) F[e] = 0.0f;
    }
#endif
    int lo[D], nbx[D];                                     // the box: first block and blocks per axis
    float* s_rec = lds + a.off_par;
    const long long nrec = area_each_box<D, BLEND>(s, lds, any, c0, c1, lo, nbx);
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

    // staging: the lattice values, the means, the counts and the block indices of the workgroup's points
    uint32_t* sv = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    uint32_t* sm = sv + per * C;
    uint32_t* sc = sm + per * C;
    uint32_t* sbk = sc + per;
    if (i < pe) {
        BlockRegs<D, C, K> R;
        long long cur_id = -1;
        float acc[C];
        int jm[D];
#pragma unroll
        for (int l = 0; l < D; ++l) jm[l] = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;
        int cnt = 0;
#pragma unroll 1
        for (int t = 0; t < ntaps; ++t) {                  // at most SAMPLE_AREA_TAPS trips
            float om[D], tp[D];
#if !SAMPLE_AREA_EACH_F_REGS
            int fo = tid * (D * D);                        // opaque to the compiler: the slot is re-read per tap, not kept
            asm volatile("" : "+v"(fo));
            const float* Fl = s_fp + fo;
#endif
#pragma unroll
            for (int m = 0; m < D; ++m) om[m] = s_tab[(nt[m] - 1) * AT + jm[m]];      // 1 <= nt[m] <= 16, 0 <= jm[m] < nt[m]
#pragma unroll
            for (int l = 0; l < D; ++l) {
                float v = xc[l];
#pragma unroll
                for (int m = 0; m < D; ++m) {
#if SAMPLE_AREA_EACH_F_REGS
                    const float f = F[l * D + m];
#else
                    const float f = Fl[l * D + m];
#endif
                    v = __fadd_rn(v, __fmul_rn(f, om[m]));
                }
                tp[l] = v;
            }
            bool carry = true;                             // the next multi-index, last axis fastest
#pragma unroll
            for (int m = D - 1; m >= 0; --m) {
                const int nx = jm[m] + 1;
                const bool wrap = nx >= nt[m];
                jm[m] = carry ? (wrap ? 0 : nx) : jm[m];
                carry = carry && wrap;
            }
            float x[D];
            int g[D], rec;
            long long id;
            if (point_locate_at<D>(s, lo, nbx, tp, g, x, id, rec)) {
                if (id != cur_id) {                        // the tap lies in another block: its record
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
                    float wn[D];                           // weight of the neighbour per axis, sd: its side
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
            sm[tid * C + c] = __float_as_uint(mean);
            sv[tid * C + c] = (a.fmt == SMOE_IMAGE_U8) ? (uint32_t)kq : __float_as_uint(kq * a.kc.scale);
        }
        sc[tid] = (uint32_t)cnt;
        sbk[tid] = (uint32_t)(int)(cin ? cid : -1);
    }
    __syncthreads();
    if (a.image != nullptr) {
        const bool u8 = a.fmt == SMOE_IMAGE_U8;
        point_store_plane<1>(p0, pe, sv, a.image, C, a.vec_img ? (u8 ? 4 : 2) : 0, u8);
    }
    if (q.mean != nullptr) point_store_plane<1>(p0, pe, sm, q.mean, C, q.vec_mean ? 2 : 0, false);
    if (q.count != nullptr) point_store_plane<1>(p0, pe, sc, q.count, 1, q.vec_cnt ? 4 : 0, true);
    if (s.block != nullptr) point_store_plane<1>(p0, pe, sbk, s.block, 1, s.vec_blk ? 2 : 0, false);
}

// The launch geometry and the LDS carve-up for checked arguments (point_layout): box | records | staging (lattice values, mean,
// count, block of a point) | offset table [16][16] | the workgroup's footprints [256][d * d] | its tap counts [256][d] bytes.
template <int D, int C, int K, bool FULL>
hipError_t sample_area_each_layout(SampleAreaEachArgs& q, long long records, RenderLayout& g) {
    constexpr int AT = SAMPLE_AREA_AXIS_TAPS;
    if (q.s.r.kc.qmode != 0 && !FULL) return hipErrorNotSupported;
    g.hl = 0;
    const hipError_t e = point_layout(D, 2 * C + 2, 1, BlendRec<D, C, K>::STRIDE, records, q.s, g);
    if (e != hipSuccess) return e;
    q.off_tab = round_up(q.s.r.off_stage + RENDER_THREADS * (2 * C + 2), 4);
    q.off_fp = q.off_tab + AT * AT;
    q.off_tap = q.off_fp + RENDER_THREADS * D * D;
    g.lds_bytes = sizeof(float) * ((size_t)q.off_tap + (size_t)(RENDER_THREADS * D / 4));
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    return hipSuccess;
}

// the instantiation for (fake-quantised graph, inverse covariance); the fake-quantised ones exist for FULL triples
template <int D, int C, int K, bool FULL, bool BLEND>
auto sample_area_each_kernel_for(bool quant, bool ic) -> void (*)(SampleAreaEachArgs) {
    if constexpr (FULL) {
        if (quant) return ic ? &sample_area_each_kernel<D, C, K, true, true, BLEND> : &sample_area_each_kernel<D, C, K, true, false, BLEND>;
    }
    if (quant) return nullptr;
    return ic ? &sample_area_each_kernel<D, C, K, false, true, BLEND> : &sample_area_each_kernel<D, C, K, false, false, BLEND>;
}

// The kernel of a planned call (geometry filled by sample_area_each_layout): the launch alone.
template <int D, int C, int K, bool FULL>
hipError_t launch_sample_area_each(const SampleAreaEachArgs& q, const RenderLayout& g, hipStream_t st) {
    const bool quant = q.s.r.kc.qmode != 0;
    bool blend = false;
    for (int l = 0; l < D; ++l) blend = blend || q.s.band[l] > 0.0f;
    const auto kern = blend ? sample_area_each_kernel_for<D, C, K, FULL, true>(quant, q.s.r.kc.inverse_cov != 0)
                            : sample_area_each_kernel_for<D, C, K, FULL, false>(quant, q.s.r.kc.inverse_cov != 0);
    if (kern == nullptr) return hipErrorNotSupported;
    return launch_decoder(kern, g.workgroups, RENDER_THREADS, g.lds_bytes, q, st);
}

}  // namespace smoe
#endif
