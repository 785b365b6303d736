// smoe_render.hip.h -- decoder: evaluate fitted block models on a separable sampling grid and store the samples at their
// place in the stitched, interleaved image [E_0, E_1(, E_2), C] (smoe_render, include/smoe_hip.h).
//
// Per block the kernel loads and derives the parameters exactly as forward_kernel does (same active rule
// `kernel_list & pis > 0`, same fake-quantised variables), then runs pixel<TRAIN = false> on every sample: gate, min-influence
// mask, expert blend, clip, lattice.  No target, no loss, no reduction, no write to `active`.
//
// Arrangement.  A workgroup of 256 lanes takes NB blocks that are neighbours along the image's innermost axis (one "grid
// line" = fixed block indices on the other axes).  A lane owns (block, sample j on the innermost axis, phase): its innermost
// coordinate is a lane constant, and it walks the tuples o of the outer sample indices with stride RP.  One step of the
// workgroup therefore completes, for RP outer tuples, the whole run of NB * m_last * C values that the blocks own on that
// image row.  The values are turned through LDS (double-buffered, one barrier per step) and leave as 16-byte non-temporal
// stores on 16-byte boundaries of the IMAGE, whatever the run's own alignment; ragged heads / tails and the crop at the
// extent go out element-wise.  uint8 output and the argmax plane take the same path with 16 values per store.
//
// HL: hoisting level of pixel<>.  The evaluation kernels pre-sum the terms of the lane-constant trailing coordinates
// (hoist_const), which fixes the order of the fused multiply-adds; the host passes the level smoe_forward would run with
// for the same handle and block count, so that a render on the training lattice is bit-identical to smoe_forward's recon.
// HL = 1 is free here (the innermost coordinate is a lane constant by construction); HL = 2 re-derives the constants when
// the lane's second-last index changes (never, when RP is a multiple of that axis' sample count: the host sees to it).
//
// argmax: first maximum among the kernels with influence, 255 where no kernel has influence on the sample.  smoe_forward
// patches such pixels with the block's first kernel that has influence anywhere on the training lattice; a render grid has
// no such block-wide notion, so the 255 STAYS here.
#ifndef SMOE_RENDER_HIP_H
#define SMOE_RENDER_HIP_H

#include "smoe_block.hip.h"

namespace smoe {

constexpr int RENDER_THREADS = 256;

// One 16-byte (ve elements) or element-wise piece [lo, hi) of a run.  st: the staged dwords (value bits, or the lattice
// index / kernel id as an integer); e0: image element of the run's first value, s0: its staged index.
template <bool U8>
__device__ __forceinline__ void render_store_piece(const uint32_t* __restrict__ st, void* __restrict__ img, long long lo,
                                                   long long hi, long long e0, int s0, int ve) {
    const uint32_t* src = st + s0 + (int)(lo - e0);
    if (ve > 1 && hi - lo == ve) {
        if constexpr (U8) {
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                w[q] = (src[4 * q] & 255u) | ((src[4 * q + 1] & 255u) << 8) | ((src[4 * q + 2] & 255u) << 16) | (src[4 * q + 3] << 24);
            const float4 v = {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
            store_stream(reinterpret_cast<float*>(static_cast<uint8_t*>(img) + lo), v);
        } else {
            const float4 v = {__uint_as_float(src[0]), __uint_as_float(src[1]), __uint_as_float(src[2]), __uint_as_float(src[3])};
            store_stream(static_cast<float*>(img) + lo, v);
        }
        return;
    }
    for (long long e = lo; e < hi; ++e) {
        const uint32_t v = src[(int)(e - lo)];
        if constexpr (U8) static_cast<uint8_t*>(img)[e] = (uint8_t)v;
        else static_cast<uint32_t*>(img)[e] = v;
    }
}

// The runs one step of the workgroup completed, from the staging buffer to the image.  cps: components per sample (C, or 1
// for the argmax plane); ve: elements per vector store (1: the plane's base is not 16-byte aligned).
template <int D, bool U8>
__device__ __forceinline__ void render_flush(const RenderArgs& a, const uint32_t* __restrict__ st, void* __restrict__ img,
                                             int cps, int ve, int it, int pass, int lb_lo, int lb_hi, int g0, int g1, int gl0) {
    const int ML = a.m[D - 1];
    const int MO = (D == 3) ? a.m[0] * a.m[1] : a.m[0];
    const bool merge = (a.CL == ML);                       // the blocks' runs adjoin: one run per outer tuple
    const int nruns = merge ? a.RP : a.RP * a.NB;
    const int maxlen = (merge ? (lb_hi - lb_lo) * ML : a.CL) * cps;
    const int cpr = (maxlen + ve - 1) / ve + 1;            // 16-byte lines a run can touch
    const long long EL = a.ext[D - 1];
    for (int w = threadIdx.x; w < nruns * cpr; w += RENDER_THREADS) {
        const int run = w / cpr;
        const int ch = w - run * cpr;
        const int r = merge ? run : run / a.NB;
        const int lbA = merge ? lb_lo : run - r * a.NB;
        if (lbA < lb_lo || lbA >= lb_hi) continue;
        const int o = it * a.RP + r;
        if (o >= MO) continue;
        long long row;
        if (D == 3) {
            const int j0 = o / a.m[1], j1 = o - j0 * a.m[1];
            const long long p0 = (long long)g0 * a.m[0] + j0, p1 = (long long)g1 * a.m[1] + j1;
            if (p0 >= a.ext[0] || p1 >= a.ext[1]) continue;
            row = p0 * a.ext[1] + p1;
        } else {
            row = (long long)g0 * a.m[0] + o;
            if (row >= a.ext[0]) continue;
        }
        const long long sA = (long long)(gl0 + lbA) * ML + (long long)pass * a.CL;      // first sample of the run on its row
        long long sE = merge ? (long long)(gl0 + lb_hi) * ML : sA + min(a.CL, ML - pass * a.CL);
        if (sE > EL) sE = EL;                                                          // positions >= extent are not written
        if (sA >= sE) continue;
        const long long e0 = (row * EL + sA) * cps, e1 = (row * EL + sE) * cps;
        const long long c0 = (e0 / ve + ch) * ve;
        if (c0 >= e1) continue;
        const long long lo = (c0 > e0) ? c0 : e0;
        const long long hi = (c0 + ve < e1) ? c0 + ve : e1;
        render_store_piece<U8>(st, img, lo, hi, e0, (r * a.NB + lbA) * a.CL * cps, ve);
    }
}

template <int D, int C, int K, int HL, bool QUANT, bool IC>
__global__ void __launch_bounds__(RENDER_THREADS) render_kernel(RenderArgs a) {
    using Lt = Layout<D, C, K>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int ML = a.m[D - 1];
    const int MO = (D == 3) ? a.m[0] * a.m[1] : a.m[0];
    const int GL = a.grid[D - 1];
    const int line = a.line0 + (int)(blockIdx.x / (unsigned)a.chunks);
    const int gl0 = (int)(blockIdx.x % (unsigned)a.chunks) * a.NB;      // first block of the workgroup on the innermost grid axis
    const int g0 = (D == 3) ? line / a.grid[1] : line;
    const int g1 = (D == 3) ? line - g0 * a.grid[1] : 0;
    // the workgroup's blocks that belong to the shard [first, first + nb): a contiguous range lb_lo .. lb_hi of its NB
    const long long id0 = (long long)line * GL + gl0;                   // image-wide index of block lb = 0
    const int lb_lo = (int)max(0LL, (long long)a.first - id0);
    const int lb_hi = (int)min((long long)min(a.NB, GL - gl0), (long long)a.first + a.nb - id0);
    if (lb_lo >= lb_hi) return;

    // LDS: axis tables | block images | staging (two buffers of values + kernel ids)
    float* s_ax = lds;
    float* s_par = lds + a.off_par;
    uint32_t* s_stage = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    const int per = a.RP * a.NB * a.CL;                                 // samples per step of the workgroup
    const int stg = per * (C + 1);
    int ax_off[D];
    {
        int o = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) { ax_off[l] = o; o += a.m[l]; }
#pragma unroll
        for (int l = 0; l < D; ++l)
            for (int i = tid; i < a.m[l]; i += RENDER_THREADS) s_ax[ax_off[l] + i] = a.ax[l][i];
    }
    for (int i = tid; i < a.NB * Lt::LP_STRIDE; i += RENDER_THREADS) {
        const int lb = i / Lt::LP_STRIDE;
        const int j = i - lb * Lt::LP_STRIDE;
        float v = 0.0f;
        if (lb >= lb_lo && lb < lb_hi) {
            const int bl = (int)(id0 + lb - a.first);                   // index into the shard's arrays
            if (j < Lt::NPAR) {
                int tensor, kern;
                long off;
                decode_slot<D, C, K>(j, bl, tensor, off, kern);
                v = pick(a.p, tensor)[off];
            } else if (j < Lt::LP_ACT + K) {
                v = (a.active == nullptr || ((a.active[bl] >> (j - Lt::LP_ACT)) & 1u)) ? 1.0f : 0.0f;
            }
        }
        s_par[i] = v;
    }
    __syncthreads();

    const int lpb = a.CL * a.RP;
    const int lb = tid / lpb;
    const int wi = tid - lb * lpb;
    const int ph = wi / a.CL;
    const int jl0 = wi - ph * a.CL;
    const bool lane_ok = lb >= lb_lo && lb < lb_hi;
    const int lbc = lane_ok ? lb : lb_lo;

    BlockRegs<D, C, K> R;
    R.load(s_par + lbc * Lt::LP_STRIDE);
    if (a.kc.qmode != 0 || a.kc.qpis != 0)
        quantize_packed<D, C, K, QUANT>(R.P, a.kc, (QUANT && a.mus_grid != nullptr) ? a.mus_grid + (size_t)(id0 + lbc - a.first) * (K * D) : nullptr);
    R.template derive<IC>(a.kc);

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
                } else {
                    x[0] = s_ax[o];
                }
                float acc[Lt::NSLOT];
#pragma unroll
                for (int j = 0; j < Lt::NSLOT; ++j) acc[j] = 0.0f;
                PixelOut<D, C, K> po;
                pixel<D, C, K, false, HL, false, IC, false>(R, a.kc, x, t0, 1.0f, acc, po);
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
            // (the next step writes the OTHER buffer while slower lanes still read this one; that step's barrier separates
            // these reads from the step after it, which writes this buffer again)
            if (a.fmt == SMOE_IMAGE_U8) render_flush<D, true>(a, sv, a.image, C, ve_img, it, pass, lb_lo, lb_hi, g0, g1, gl0);
            else render_flush<D, false>(a, sv, a.image, C, ve_img, it, pass, lb_lo, lb_hi, g0, g1, gl0);
            if (a.argmax != nullptr) render_flush<D, true>(a, sa, a.argmax, 1, ve_arg, it, pass, lb_lo, lb_hi, g0, g1, gl0);
            buf ^= 1;
        }
    }
}

// Launch geometry: CL concurrent innermost samples per block, RP outer tuples per step, NB blocks per workgroup.
// lanes: the lanes-per-block tiling the evaluation takes for this many blocks (16 / 32 / 64).
inline void render_geometry(int D, const int* m, int grid_last, int lanes, int hl, RenderArgs& a) {
    const int ML = m[D - 1];
    const long MO = (D == 3) ? (long)m[0] * m[1] : m[0];
    const int cl = (ML < RENDER_THREADS) ? ML : RENDER_THREADS;
    int rp = (lanes > cl) ? lanes / cl : 1;
    if (D == 3 && hl == 2 && rp % m[1] != 0) {             // keep the second-last index a lane constant where it fits
        const long up = ((long)rp + m[1] - 1) / m[1] * m[1];
        if (up * cl <= RENDER_THREADS) rp = (int)up;
    }
    if (rp > MO) rp = (int)MO;
    if (rp * cl > RENDER_THREADS) rp = RENDER_THREADS / cl;
    if (rp < 1) rp = 1;
    int nb = RENDER_THREADS / (cl * rp);
    if (nb < 1) nb = 1;
    if (nb > grid_last) nb = grid_last;
    a.CL = cl; a.RP = rp; a.NB = nb;
    a.chunks = (grid_last + nb - 1) / nb;
}

template <int D, int C, int K, bool FULL>
hipError_t launch_render(const RenderArgs& a0, int hl, int lanes, hipStream_t st) {
    using Lt = Layout<D, C, K>;
    RenderArgs a = a0;
    const bool ic = a.kc.inverse_cov != 0;
    const bool q = a.kc.qmode != 0;
    if (q && !FULL) return hipErrorNotSupported;
    if (hl > D - 1) hl = D - 1;
    if (q && hl > 1) hl = 1;                               // as the quantised evaluation (resolve_fwd)
    void (*kern)(RenderArgs) = nullptr;
#define SMOE_RENDER_PICK(H)                                                                                            \
    do {                                                                                                               \
        if constexpr (FULL && (H) <= 1) {                                                                              \
            if (q) kern = ic ? render_kernel<D, C, K, (H), true, true> : render_kernel<D, C, K, (H), true, false>;     \
        }                                                                                                              \
        if (!q) kern = ic ? render_kernel<D, C, K, (H), false, true> : render_kernel<D, C, K, (H), false, false>;      \
    } while (0)
    if (hl == 0) SMOE_RENDER_PICK(0);
    if (hl == 1) SMOE_RENDER_PICK(1);
    if constexpr (D == 3) {
        if (hl == 2) SMOE_RENDER_PICK(2);
    }
#undef SMOE_RENDER_PICK
    if (kern == nullptr) return hipErrorNotSupported;
    render_geometry(D, a.m, a.grid[D - 1], lanes, hl, a);
    long msum = 0;
    for (int l = 0; l < D; ++l) msum += a.m[l];
    if (msum > 32768) return hipErrorNotSupported;         // the axis tables live in LDS
    a.off_par = round_up((int)msum, 4);
    a.off_stage = a.off_par + a.NB * Lt::LP_STRIDE;
    const size_t shm = sizeof(float) * ((size_t)a.off_stage + 2u * (size_t)a.RP * a.NB * a.CL * (C + 1));
    if (shm > 160u * 1024u) return hipErrorNotSupported;
    const long long GL = a.grid[D - 1];
    const long long line_lo = a.first / GL, line_hi = ((long long)a.first + a.nb - 1) / GL;
    a.line0 = (int)line_lo;
    const long long wgs = (line_hi - line_lo + 1) * a.chunks;
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e = allow_lds(reinterpret_cast<const void*>(kern), shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(RENDER_THREADS), shm, st, a);
    return hipGetLastError();
}

}  // namespace smoe
#endif
