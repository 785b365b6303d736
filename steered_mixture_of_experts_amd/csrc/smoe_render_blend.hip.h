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
    const int ML = a.m[D - 1];
    const int MO = (D == 3) ? a.m[0] * a.m[1] : a.m[0];
    const int GL = a.grid[D - 1];
    const int line = a.line0 + (int)(blockIdx.x / (unsigned)a.chunks);
    const int gl0 = (int)(blockIdx.x % (unsigned)a.chunks) * a.NB;
    const int g0 = (D == 3) ? line / a.grid[1] : line;
    const int g1 = (D == 3) ? line - g0 * a.grid[1] : 0;
    const long long id0 = (long long)line * GL + gl0;
    const int lb_lo = (int)max(0LL, (long long)a.first - id0);
    const int lb_hi = (int)min((long long)min(a.NB, GL - gl0), (long long)a.first + a.nb - id0);
    if (lb_lo >= lb_hi) return;

    // LDS: axis tables | neighbour-weight tables | block records | staging (two buffers of values + kernel ids)
    float* s_ax = lds;
    float* s_w = lds + b.off_w;
    float* s_rec = lds + a.off_par;
    uint32_t* s_stage = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    const int per = a.RP * a.NB * a.CL;
    const int stg = per * (C + 1);
    int ax_off[D];
    {
        int o = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) { ax_off[l] = o; o += a.m[l]; }
#pragma unroll
        for (int l = 0; l < D; ++l)
            for (int i = tid; i < a.m[l]; i += RENDER_THREADS) {
                const float u = a.ax[l][i];
                float w = 0.0f;
                if (b.band[l] > 0.0f) {
                    const float hi = fminf(fmaxf(0.5f * (1.0f + (u - b.s1[l]) / b.band[l]), 0.0f), 1.0f);
                    const float lo = fminf(fmaxf(0.5f * (1.0f + (b.s0[l] - u) / b.band[l]), 0.0f), 1.0f);
                    w = (hi > 0.0f) ? hi : -lo;
                }
                s_ax[ax_off[l] + i] = u;
                s_w[ax_off[l] + i] = w;
            }
    }
    const int ni = a.NB + 2;
    const int nrec = Rc::OUTER * ni;
    for (int i = tid; i < nrec * Lt::LP_STRIDE; i += RENDER_THREADS) {
        const int rec = i / Lt::LP_STRIDE;
        const int j = i - rec * Lt::LP_STRIDE;
        const long long id = record_block<D>(a, rec, ni, g0, g1, gl0);
        float v = 0.0f;
        if (id >= 0) {
            if (j < Lt::NPAR) {
                int tensor, kern;
                long off;
                decode_slot<D, C, K>(j, (int)id, tensor, off, kern);
                v = pick(a.p, tensor)[off];
            } else if (j < Lt::LP_ACT + K) {
                v = (a.active == nullptr || ((a.active[id] >> (j - Lt::LP_ACT)) & 1u)) ? 1.0f : 0.0f;
            }
        }
        s_rec[rec * Rc::STRIDE + j] = v;
    }
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

    const int lpb = a.CL * a.RP;
    const int lb = tid / lpb;
    const int wi = tid - lb * lpb;
    const int ph = wi / a.CL;
    const int jl0 = wi - ph * a.CL;
    const bool lane_ok = lb >= lb_lo && lb < lb_hi;
    const int lbc = lane_ok ? lb : lb_lo;
    const int own_rec = Rc::CENTRE * ni + lbc + 1;
    const int rec_step0 = (D == 3) ? 3 * ni : ni;          // record index step per block along axis 0 (axis 1 of three: ni)

    BlockRegs<D, C, K> R;
    load_record<D, C, K>(R, s_rec + own_rec * Rc::STRIDE);

    float t0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t0[c] = 0.0f;
    const int npass = (ML + a.CL - 1) / a.CL;
    const int nit = (MO + a.RP - 1) / a.RP;
    const int ve_img = a.vec_img ? ((a.fmt == SMOE_IMAGE_U8) ? 16 : 4) : 1;
    const int ve_arg = a.vec_arg ? 16 : 1;
    int buf = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const int jl = jl0 + pass * a.CL;
        const bool col_ok = lane_ok && jl < ML;
        float xc[D];
#pragma unroll
        for (int l = 0; l < D; ++l) xc[l] = 0.0f;
        xc[D - 1] = s_ax[ax_off[D - 1] + min(jl, ML - 1)];
        float wn[D];                                       // weight of the neighbour per axis, sd: its side
        int sd[D];
        {
            const float w = s_w[ax_off[D - 1] + min(jl, ML - 1)];
            sd[D - 1] = (w > 0.0f) ? 1 : -1;
            const int gn = gl0 + lbc + sd[D - 1];
            wn[D - 1] = (gn >= 0 && gn < GL) ? fabsf(w) : 0.0f;
        }
        int cur1 = -1;
        if (HL == 1) hoist_const<D, C, K, HL, IC>(R, xc);
        for (int it = 0; it < nit; ++it) {
            const int o = it * a.RP + ph;
            uint32_t* sv = s_stage + buf * stg;
            uint32_t* sa = sv + per * C;
            if (col_ok && o < MO) {
                float x[D];
                x[D - 1] = xc[D - 1];
                if (D == 3) {
                    const int j0 = o / a.m[1], j1 = o - j0 * a.m[1];
                    x[0] = s_ax[j0];
                    x[1] = s_ax[ax_off[1] + j1];
                    if (HL == 2 && j1 != cur1) {
                        xc[1] = x[1];
                        hoist_const<D, C, K, HL, IC>(R, xc);
                        cur1 = j1;
                    }
                    const float w0 = s_w[j0], w1 = s_w[ax_off[1] + j1];
                    sd[0] = (w0 > 0.0f) ? 1 : -1;
                    sd[1] = (w1 > 0.0f) ? 1 : -1;
                    wn[0] = (g0 + sd[0] >= 0 && g0 + sd[0] < a.grid[0]) ? fabsf(w0) : 0.0f;
                    wn[1] = (g1 + sd[1] >= 0 && g1 + sd[1] < a.grid[1]) ? fabsf(w1) : 0.0f;
                } else {
                    x[0] = s_ax[o];
                    const float w0 = s_w[o];
                    sd[0] = (w0 > 0.0f) ? 1 : -1;
                    wn[0] = (g0 + sd[0] >= 0 && g0 + sd[0] < a.grid[0]) ? fabsf(w0) : 0.0f;
                }
                float acc[Lt::NSLOT];
#pragma unroll
                for (int j = 0; j < Lt::NSLOT; ++j) acc[j] = 0.0f;
                PixelOut<D, C, K> po;
                pixel<D, C, K, false, HL, false, IC, false>(R, a.kc, x, t0, 1.0f, acc, po);
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
                const int si = (ph * a.NB + lb) * a.CL + jl0;
                if (a.fmt == SMOE_IMAGE_U8) {
#pragma unroll
                    for (int c = 0; c < C; ++c) sv[si * C + c] = (uint32_t)po.kq[c];
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) sv[si * C + c] = __float_as_uint(po.q[c]);
                }
                if (a.argmax != nullptr) {
                    float best = 0.0f;
                    uint32_t arg = 255u;
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (po.wt[k] > best) { best = po.wt[k]; arg = (uint32_t)k; }
                    sa[si] = arg;
                }
            }
            __syncthreads();
            if (a.fmt == SMOE_IMAGE_U8) render_flush<D, true>(a, sv, a.image, C, ve_img, it, pass, lb_lo, lb_hi, g0, g1, gl0);
            else render_flush<D, false>(a, sv, a.image, C, ve_img, it, pass, lb_lo, lb_hi, g0, g1, gl0);
            if (a.argmax != nullptr) render_flush<D, true>(a, sa, a.argmax, 1, ve_arg, it, pass, lb_lo, lb_hi, g0, g1, gl0);
            buf ^= 1;
        }
    }
}

template <int D, int C, int K, bool FULL>
hipError_t launch_render_blend(const RenderBlendArgs& b0, int hl, int lanes, hipStream_t st) {
    using Rc = BlendRec<D, C, K>;
    RenderBlendArgs b = b0;
    RenderArgs& a = b.r;
    const bool ic = a.kc.inverse_cov != 0;
    const bool q = a.kc.qmode != 0;
    if (q && !FULL) return hipErrorNotSupported;
    if (hl > D - 1) hl = D - 1;
    if (q && hl > 1) hl = 1;                               // as launch_render: the own block's samples follow smoe_render's order
    void (*kern)(RenderBlendArgs) = nullptr;
#define SMOE_BLEND_PICK(H)                                                                                                   \
    do {                                                                                                                     \
        if constexpr (FULL && (H) <= 1) {                                                                                    \
            if (q) kern = ic ? render_blend_kernel<D, C, K, (H), true, true> : render_blend_kernel<D, C, K, (H), true, false>;   \
        }                                                                                                                    \
        if (!q) kern = ic ? render_blend_kernel<D, C, K, (H), false, true> : render_blend_kernel<D, C, K, (H), false, false>;    \
    } while (0)
    if (hl == 0) SMOE_BLEND_PICK(0);
    if (hl == 1) SMOE_BLEND_PICK(1);
    if constexpr (D == 3) {
        if (hl == 2) SMOE_BLEND_PICK(2);
    }
#undef SMOE_BLEND_PICK
    if (kern == nullptr) return hipErrorNotSupported;
    render_geometry(D, a.m, a.grid[D - 1], lanes, hl, a);
    // the records of 3^(d-1) x (NB + 2) blocks: fewer blocks per workgroup where they would take more than 48 KB, the lanes
    // that frees go to further outer sample tuples (a sample's arithmetic does not depend on the geometry)
    const int nb_plain = a.NB;
    while (a.NB > 1 && sizeof(float) * (size_t)Rc::OUTER * (a.NB + 2) * Rc::STRIDE > 48u * 1024u) --a.NB;
    if (a.NB < nb_plain) {
        const long MO = (D == 3) ? (long)a.m[0] * a.m[1] : a.m[0];
        long rp = RENDER_THREADS / (a.CL * a.NB);
        if (rp > MO) rp = MO;
        if (rp > a.RP) a.RP = (int)rp;
    }
    a.chunks = (a.grid[D - 1] + a.NB - 1) / a.NB;
    long msum = 0;
    for (int l = 0; l < D; ++l) msum += a.m[l];
    if (msum > 16384) return hipErrorNotSupported;         // the coordinate and the weight tables live in LDS (smoe_render: 32768)
    b.off_w = round_up((int)msum, 4);
    a.off_par = 2 * b.off_w;
    a.off_stage = a.off_par + Rc::OUTER * (a.NB + 2) * Rc::STRIDE;
    const size_t shm = sizeof(float) * ((size_t)a.off_stage + 2u * (size_t)a.RP * a.NB * a.CL * (C + 1));
    if (shm > 160u * 1024u) return hipErrorNotSupported;
    const long long GL = a.grid[D - 1];
    const long long line_lo = a.first / GL, line_hi = ((long long)a.first + a.nb - 1) / GL;
    a.line0 = (int)line_lo;
    const long long wgs = (line_hi - line_lo + 1) * a.chunks;
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e = allow_lds(reinterpret_cast<const void*>(kern), shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(RENDER_THREADS), shm, st, b);
    return hipGetLastError();
}

}  // namespace smoe
#endif
