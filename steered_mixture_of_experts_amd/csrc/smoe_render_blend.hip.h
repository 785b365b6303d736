// smoe_render_blend.hip.h -- seam-free decoder: smoe_render's samples, cross-faded with the neighbouring blocks' models in a
// band around every block border (smoe_render_blend, include/smoe_hip.h).
//
// Definition.  Per axis l a sample with block-unit coordinate u has the neighbour weight
//     w_hi = clamp(0.5 * (1 + (u - s1) / b), 0, 1)     s1 = 1 + 0.5 / (n - 1)   (the seam towards block g + 1)
//     w_lo = clamp(0.5 * (1 + (s0 - u) / b), 0, 1)     s0 =   - 0.5 / (n - 1)   (the seam towards block g - 1)
// with b = blend / (n - 1) the half-width of the band in block units; at most one of the two is positive (blend <= n / 2),
// a neighbour outside the image gets 0 and the own block 1 - w.  The weight W of each of the up to 2^d blocks around a sample
// is the product over the axes; a block with W > 0 is evaluated at ITS coordinate of the sample (u -+ n / (n - 1) on the axes
// where it is the neighbour), exactly as render_kernel evaluates a block; blocks without a kernel of influence on the sample
// are dropped; the sample is sum W clip(y) / sum W over the rest (0 when none is left), put on the lattice once.
//
// Arrangement: render_kernel's.  A workgroup takes NB blocks along the innermost grid axis, a lane owns (block, innermost
// sample, phase) and walks the outer sample tuples; the values leave through the same LDS staging and 16-byte stores
// (render_flush).  What is new:
//  * the DERIVED records (fake-quantised packed parameters, A', c, coef: what BlockRegs::load / quantize_packed / derive
//    leave) of the 3^(d-1) x (NB + 2) blocks on and around the workgroup's grid line sit in LDS, made once per workgroup by
//    one lane per record; a lane reads its own block's record into registers before the loop and a neighbour's when it
//    needs one;
//  * per axis a table of the signed neighbour weight of every local sample index (> 0: towards g + 1, < 0: towards g - 1)
//    sits beside the coordinate tables, so the loop pays two LDS reads per sample for the weights;
//  * a sample is first evaluated exactly as in render_kernel (same hoisting level, same order of fused multiply-adds):
//    with every neighbour weight 0 that result is stored, bit for bit smoe_render's.  Behind a wavefront-wide vote
//    (`__ballot(band)`) the lanes inside a band re-form their own pre-clip blend, then run one non-unrolled loop over the
//    2^d - 1 corners, each corner behind its own vote: a wavefront with no lane in a band pays one evaluation per sample,
//    one on a straight seam two, only the wavefronts on a corner more.  Neighbours are evaluated without hoisting (their
//    order of operations is not tied to anything).  With this lane mapping a wavefront holds whole rows of its blocks, so
//    in practice every wavefront has lanes in the innermost band and passes the first vote (measured cost).
// argmax is the own block's, as in smoe_render.
#ifndef SMOE_RENDER_BLEND_HIP_H
#define SMOE_RENDER_BLEND_HIP_H

#include "smoe_render.hip.h"

namespace smoe {

// LDS record of one block: Layout's block image (after quantize_packed and derive), then A', c and coef of BlockRegs
template <int D, int C, int K>
struct BlendRec {
    using Lt = Layout<D, C, K>;
    static constexpr int O_AS = Lt::LP_STRIDE;
    static constexpr int O_CZ = O_AS + K * Lt::TRI;
    static constexpr int O_COEF = O_CZ + K * D;
    static constexpr int STRIDE = round_up(O_COEF + K, 4);
    static constexpr int OUTER = (D == 3) ? 9 : 3;        // records per innermost position: the grid lines around the own one
    static constexpr int CENTRE = (D == 3) ? 4 : 1;
};

template <int D, int C, int K>
__device__ __forceinline__ void store_record(const BlockRegs<D, C, K>& R, float* __restrict__ rec) {
    using Rc = BlendRec<D, C, K>;
#pragma unroll
    for (int i = 0; i < Rc::Lt::LP_STRIDE; ++i) rec[i] = R.P[i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < Rc::Lt::TRI; ++i) rec[Rc::O_AS + k * Rc::Lt::TRI + i] = R.As[k][i];
#pragma unroll
        for (int m = 0; m < D; ++m) rec[Rc::O_CZ + k * D + m] = R.cz[k][m];
        rec[Rc::O_COEF + k] = R.coef[k];
    }
}

template <int D, int C, int K>
__device__ __forceinline__ void load_record(BlockRegs<D, C, K>& R, const float* __restrict__ rec) {
    using Rc = BlendRec<D, C, K>;
    R.load(rec);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < Rc::Lt::TRI; ++i) R.As[k][i] = rec[Rc::O_AS + k * Rc::Lt::TRI + i];
#pragma unroll
        for (int m = 0; m < D; ++m) R.cz[k][m] = rec[Rc::O_CZ + k * D + m];
        R.coef[k] = rec[Rc::O_COEF + k];
    }
}

// image-wide index of the block behind record `rec` of the workgroup (-1: outside the block grid).  Records are ordered
// [grid line offset (d0 + 1)(* 3 + d1 + 1)][innermost position gl0 - 1 .. gl0 + NB]
template <int D>
__device__ __forceinline__ long long record_block(const RenderArgs& a, int rec, int ni, int g0, int g1, int gl0) {
    const int oc = rec / ni;
    const int gi = gl0 - 1 + (rec - oc * ni);
    if (gi < 0 || gi >= a.grid[D - 1]) return -1;
    if (D == 3) {
        const int h0 = g0 + oc / 3 - 1, h1 = g1 + oc % 3 - 1;
        if (h0 < 0 || h0 >= a.grid[0] || h1 < 0 || h1 >= a.grid[1]) return -1;
        return ((long long)h0 * a.grid[1] + h1) * a.grid[2] + gi;
    }
    const int h0 = g0 + oc - 1;
    if (h0 < 0 || h0 >= a.grid[0]) return -1;
    return (long long)h0 * a.grid[1] + gi;
}

// the pre-clip blend of pixel<> from its masked gate: the same fused multiply-adds in the same order (pixel<> keeps y to itself)
template <int D, int C, int K, int HL>
__device__ __forceinline__ void blend_y(const BlockRegs<D, C, K>& R, const float (&x)[D], const float (&wt)[K], float (&y)[C]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float ee = (HL > 0) ? R.he[k][c] : R.nu(k, c);
#pragma unroll
            for (int l = 0; l < D - HL; ++l) ee = fmaf(R.ga(k, l, c), x[l], ee);
            y[c] = (k == 0) ? wt[k] * ee : fmaf(wt[k], ee, y[c]);
        }
}

template <int K>
__device__ __forceinline__ bool has_influence(const float (&wt)[K]) {
    float mx = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, wt[k]);
    return mx > 0.0f;
}

template <int D, int C, int K, int HL, bool QUANT, bool IC>
__global__ void __launch_bounds__(RENDER_THREADS) render_blend_kernel(RenderBlendArgs b) {
    using Lt = Layout<D, C, K>;
    using Rc = BlendRec<D, C, K>;
    const RenderArgs& a = b.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    RenderFrame<D> f;
    if (!f.place(a)) return;
    const int g0 = f.g0, g1 = f.g1, gl0 = f.gl0;

    // LDS: axis tables | neighbour-weight tables | block records | staging (two buffers of values + kernel ids)
    float* s_ax = lds;
    float* s_w = lds + b.off_w;
    float* s_rec = lds + a.off_par;
    render_load_axes<D>(a, f, [&](int l, int slot, float u) {
        float w = 0.0f;
        if (b.band[l] > 0.0f) {
            const float hi = fminf(fmaxf(0.5f * (1.0f + (u - b.s1[l]) / b.band[l]), 0.0f), 1.0f);
            const float lo = fminf(fmaxf(0.5f * (1.0f + (b.s0[l] - u) / b.band[l]), 0.0f), 1.0f);
            w = (hi > 0.0f) ? hi : -lo;
        }
        s_ax[slot] = u;
        s_w[slot] = w;
    });
    const int ni = a.NB + 2;
    const int nrec = Rc::OUTER * ni;
    render_load_images<D, C, K, Rc::STRIDE>(a, s_rec, nrec, [&](int rec, long long& id) {
        id = record_block<D>(a, rec, ni, g0, g1, gl0);
        return id >= 0;
    });
    __syncthreads();
    // one lane per record: what every lane of render_kernel does for its block, kept for all of them
    for (int rec = tid; rec < nrec; rec += RENDER_THREADS) {
        const long long id = record_block<D>(a, rec, ni, g0, g1, gl0);
        if (id < 0) continue;
        BlockRegs<D, C, K> T;
        T.load(s_rec + rec * Rc::STRIDE);
        if (a.kc.qmode != 0 || a.kc.qpis != 0)
            quantize_packed<D, C, K, QUANT>(T.P, a.kc, (QUANT && a.mus_grid != nullptr) ? a.mus_grid + (size_t)id * (K * D) : nullptr);
        T.template derive<IC>(a.kc);
        store_record<D, C, K>(T, s_rec + rec * Rc::STRIDE);
    }
    __syncthreads();

    const RenderLane n = render_lane<D>(a, f);
    const int own_rec = Rc::CENTRE * ni + n.lbc + 1;
    const int rec_step0 = (D == 3) ? 3 * ni : ni;          // record index step per block along axis 0 (axis 1 of three: ni)

    BlockRegs<D, C, K> R;
    load_record<D, C, K>(R, s_rec + own_rec * Rc::STRIDE);

    float t0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t0[c] = 0.0f;
    RenderWalk<D, C> w;
    w.begin(a, f, lds);
    for (int pass = 0; pass < w.npass; ++pass) {
        float xc[D];
        int cur1;
        const int jl = render_begin_pass<D, C, K, HL, IC>(a, f, n, s_ax, pass, R, xc, cur1);
        const bool col_ok = n.ok && jl < f.ML;
        float wn[D];                                       // weight of the neighbour per axis, sd: its side
        int sd[D];
        {
            const float sw = s_w[f.ax_off[D - 1] + min(jl, f.ML - 1)];
            sd[D - 1] = (sw > 0.0f) ? 1 : -1;
            const int gn = gl0 + n.lbc + sd[D - 1];
            wn[D - 1] = (gn >= 0 && gn < f.GL) ? fabsf(sw) : 0.0f;
        }
        for (int it = 0; it < w.nit; ++it) {
            const int o = it * a.RP + n.ph;
            if (col_ok && o < f.MO) {
                float x[D];
                int jo[D - 1];
                render_fetch_coords<D, C, K, HL, IC>(a, f, s_ax, o, R, xc, cur1, x, jo);
                if (D == 3) {
                    const float w0 = s_w[jo[0]], w1 = s_w[f.ax_off[1] + jo[D - 2]];
                    sd[0] = (w0 > 0.0f) ? 1 : -1;
                    sd[1] = (w1 > 0.0f) ? 1 : -1;
                    wn[0] = (g0 + sd[0] >= 0 && g0 + sd[0] < a.grid[0]) ? fabsf(w0) : 0.0f;
                    wn[1] = (g1 + sd[1] >= 0 && g1 + sd[1] < a.grid[1]) ? fabsf(w1) : 0.0f;
                } else {
                    const float w0 = s_w[jo[0]];
                    sd[0] = (w0 > 0.0f) ? 1 : -1;
                    wn[0] = (g0 + sd[0] >= 0 && g0 + sd[0] < a.grid[0]) ? fabsf(w0) : 0.0f;
                }
                PixelOut<D, C, K> po;
                render_eval<D, C, K, HL, IC>(a, R, x, po);
                bool band = false;
#pragma unroll
                for (int l = 0; l < D; ++l) band = band || (wn[l] > 0.0f);
                if (__ballot(band) != 0ull) {              // wave-uniform: no lane of the wavefront lies in a band -> nothing below
                    if (band) {
                        float y[C], num[C];
                        blend_y<D, C, K, HL>(R, x, po.wt, y);
                        float wo = 1.0f;
#pragma unroll
                        for (int l = 0; l < D; ++l) wo *= 1.0f - wn[l];
                        float den = has_influence<K>(po.wt) ? wo : 0.0f;
#pragma unroll
                        for (int c = 0; c < C; ++c) num[c] = den * __builtin_amdgcn_fmed3f(y[c], 0.0f, a.kc.nudged_max);
#pragma unroll 1
                        for (int cm = 1; cm < (1 << D); ++cm) {        // the corners: bit l = the neighbour on axis l
                            float W = 1.0f;
                            float xn[D];
                            int rec = own_rec;
#pragma unroll
                            for (int l = 0; l < D; ++l) {
                                const bool nb = ((cm >> l) & 1) != 0;
                                const int step = (l == D - 1) ? 1 : ((l == 0) ? rec_step0 : ni);
                                W *= nb ? wn[l] : 1.0f - wn[l];
                                xn[l] = nb ? x[l] - (float)sd[l] * b.pitch[l] : x[l];
                                rec += nb ? sd[l] * step : 0;
                            }
                            if (__ballot(W > 0.0f) == 0ull) continue;  // wave-uniform
                            if (W > 0.0f) {
                                BlockRegs<D, C, K> N;
                                load_record<D, C, K>(N, s_rec + rec * Rc::STRIDE);
                                float accn[Lt::NSLOT];
#pragma unroll
                                for (int j = 0; j < Lt::NSLOT; ++j) accn[j] = 0.0f;
                                PixelOut<D, C, K> pn;
                                pixel<D, C, K, false, 0, false, IC, false>(N, a.kc, xn, t0, 1.0f, accn, pn);
                                if (has_influence<K>(pn.wt)) {
                                    float yn[C];
                                    blend_y<D, C, K, 0>(N, xn, pn.wt, yn);
                                    den += W;
#pragma unroll
                                    for (int c = 0; c < C; ++c)
                                        num[c] = fmaf(W, __builtin_amdgcn_fmed3f(yn[c], 0.0f, a.kc.nudged_max), num[c]);
                                }
                            }
                        }
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float v = (den > 0.0f) ? num[c] / den : 0.0f;
                            po.kq[c] = floorf(fmaf(v, a.kc.inv_scale, 0.5f));
                            po.q[c] = po.kq[c] * a.kc.scale;
                        }
                    }
                }
                render_stage_sample<D, C, K>(a, n, w, po);
            }
            render_flush_step<D, C>(a, f, w, it, pass);
        }
    }
}

template <int D, int C, int K>
struct RenderBlendFamily {
    using Rc = BlendRec<D, C, K>;
    template <int HL, bool QUANT, bool IC>
    static auto kernel() -> void (*)(RenderBlendArgs) { return &render_blend_kernel<D, C, K, HL, QUANT, IC>; }
    // the records of 3^(d-1) x (NB + 2) blocks, at most 48 KB of them; the coordinate and the weight table of every axis
    static constexpr RenderRecords records() { return {Rc::STRIDE, Rc::OUTER, 2, 2, 48u * 1024u}; }
};

template <int D, int C, int K, bool FULL>
hipError_t render_blend_layout(RenderBlendArgs& b, int hl, int lanes, RenderLayout& g) {
    return render_layout(D, C, FULL, RenderBlendFamily<D, C, K>::records(), b.r, &b.off_w, hl, lanes, g);
}

// (the own block's samples follow smoe_render's order of operations: the same hoisting clamps, the same geometry rules)
template <int D, int C, int K, bool FULL>
hipError_t launch_render_blend(const RenderBlendArgs& b0, int hl, int lanes, hipStream_t st) {
    RenderBlendArgs b = b0;
    return launch_block_decoder<RenderBlendFamily<D, C, K>, D, FULL>(b, b.r, hl, lanes, st, &render_blend_layout<D, C, K, FULL>);
}

}  // namespace smoe
#endif
