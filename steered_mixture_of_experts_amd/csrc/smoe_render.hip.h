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

// Piece `ch` of the run [e0, e1) of image elements, whose first value is staged at st[s0]: the 16-byte line (ve = 1 << vs
// elements) number `ch`, counted from the line e0 lies in, cut to the run.  Nothing where the run ends before that line.
template <bool U8>
__device__ __forceinline__ void render_store_run(const uint32_t* __restrict__ st, void* __restrict__ img, long long e0,
                                                 long long e1, int s0, int vs, int ch) {
    const int ve = 1 << vs;
    const long long c0 = ((e0 >> vs) + ch) << vs;            // (a 64-bit division by ve otherwise)
    if (c0 >= e1) return;
    const long long lo = (c0 > e0) ? c0 : e0;
    const long long hi = (c0 + ve < e1) ? c0 + ve : e1;
    render_store_piece<U8>(st, img, lo, hi, e0, s0, ve);
}

// First maximum among the kernels with influence, the decoders' kernel-id plane: start from (0, the plane's marker for
// "no kernel has influence"), then offer the masked gates in ascending kernel order.
template <typename Id>
__device__ __forceinline__ void first_max_init(float& best, Id& arg, Id none) {
    best = 0.0f;
    arg = none;
}

template <typename Id>
__device__ __forceinline__ void first_max_take(float& best, Id& arg, float wt, Id id) {
    if (wt > best) { best = wt; arg = id; }
}

// ---- the frame of the block decoders (render_kernel, render_blend_kernel) ---------------------------------------------------
// The workgroup's place: its grid line (g0, g1), the first of its NB blocks on the innermost grid axis (gl0; id0 = that block's
// image-wide index) and the contiguous range lb_lo .. lb_hi of the NB that belongs to the shard [first, first + nb).
template <int D>
struct RenderFrame {
    int ML, MO, GL;               // samples per block on the innermost axis / on the outer axes together; blocks per grid line
    int g0, g1, gl0;
    long long id0;
    int lb_lo, lb_hi;
    int ax_off[D];                // offset of each axis' table in the LDS tables

    // false: none of the workgroup's blocks belongs to the shard
    __device__ __forceinline__ bool place(const RenderArgs& a) {
        ML = a.m[D - 1];
        MO = (D == 3) ? a.m[0] * a.m[1] : a.m[0];
        GL = a.grid[D - 1];
        const int line = a.line0 + (int)(blockIdx.x / (unsigned)a.chunks);
        gl0 = (int)(blockIdx.x % (unsigned)a.chunks) * a.NB;
        g0 = (D == 3) ? line / a.grid[1] : line;
        g1 = (D == 3) ? line - g0 * a.grid[1] : 0;
        id0 = (long long)line * GL + gl0;
        lb_lo = (int)max(0LL, (long long)a.first - id0);
        lb_hi = (int)min((long long)min(a.NB, GL - gl0), (long long)a.first + a.nb - id0);
        int o = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) { ax_off[l] = o; o += a.m[l]; }
        return lb_lo < lb_hi;
    }
};

// A lane owns (block lb of the workgroup, innermost sample jl0 of a pass, phase ph over the outer tuples of a step).  Lanes
// of a block outside the shard compute on block lbc and store nothing.
struct RenderLane {
    int lb, ph, jl0, lbc;
    bool ok;
};

template <int D>
__device__ __forceinline__ RenderLane render_lane(const RenderArgs& a, const RenderFrame<D>& f) {
    RenderLane n;
    const int tid = threadIdx.x;
    const int lpb = a.CL * a.RP;
    n.lb = tid / lpb;
    const int wi = tid - n.lb * lpb;
    n.ph = wi / a.CL;
    n.jl0 = wi - n.ph * a.CL;
    n.ok = n.lb >= f.lb_lo && n.lb < f.lb_hi;
    n.lbc = n.ok ? n.lb : f.lb_lo;
    return n;
}

// The per-axis coordinate tables into LDS: put(l, slot, u) stores coordinate u of axis l (and what goes with it) at `slot`.
template <int D, typename Put>
__device__ __forceinline__ void render_load_axes(const RenderArgs& a, const RenderFrame<D>& f, Put&& put) {
#pragma unroll
    for (int l = 0; l < D; ++l)
        for (int i = threadIdx.x; i < a.m[l]; i += RENDER_THREADS) put(l, f.ax_off[l] + i, a.ax[l][i]);
}

// The block images (Layout's packed parameters and the `active` flags, as forward_kernel loads them) of nrec LDS records,
// STRIDE floats apart: block_of(rec, bl) says whether a block is behind record `rec` and sets its index bl into a.p / a.active.
template <int D, int C, int K, int STRIDE, typename BlockOf>
__device__ __forceinline__ void render_load_images(const RenderArgs& a, float* __restrict__ s_rec, int nrec, BlockOf&& block_of) {
    using Lt = Layout<D, C, K>;
    for (int i = threadIdx.x; i < nrec * Lt::LP_STRIDE; i += RENDER_THREADS) {
        const int rec = i / Lt::LP_STRIDE;
        const int j = i - rec * Lt::LP_STRIDE;
        float v = 0.0f;
        long long bl;
        if (block_of(rec, bl)) {
            if (j < Lt::NPAR) {
                int tensor, kern;
                long off;
                decode_slot<D, C, K>(j, (int)bl, tensor, off, kern);
                v = pick(a.p, tensor)[off];
            } else if (j < Lt::LP_ACT + K) {
                v = (a.active == nullptr || ((a.active[bl] >> (j - Lt::LP_ACT)) & 1u)) ? 1.0f : 0.0f;
            }
        }
        s_rec[rec * STRIDE + j] = v;
    }
}

// The staging of a block decoder's steps: the two buffers in turn, and how their runs leave
template <int D, int C>
struct RenderWalk {
    uint32_t* s_stage;
    int per, stg;                 // samples / staged dwords (values + kernel ids) per step of the workgroup
    int npass, nit;
    int vs_img, vs_arg;           // log2 of the elements per 16-byte store of the image / the kernel-id plane (0: element-wise)
    int buf;

    __device__ __forceinline__ void begin(const RenderArgs& a, const RenderFrame<D>& f, float* lds) {
        s_stage = reinterpret_cast<uint32_t*>(lds + a.off_stage);
        per = a.RP * a.NB * a.CL;
        stg = per * (C + 1);
        npass = (f.ML + a.CL - 1) / a.CL;
        nit = (f.MO + a.RP - 1) / a.RP;
        vs_img = a.vec_img ? ((a.fmt == SMOE_IMAGE_U8) ? 4 : 2) : 0;
        vs_arg = a.vec_arg ? 4 : 0;
        buf = 0;
    }
    __device__ __forceinline__ uint32_t* values() const { return s_stage + buf * stg; }
    __device__ __forceinline__ uint32_t* ids() const { return values() + per * C; }
};

// A pass over the innermost axis begins: the lane's sample jl on it (returned; the lane has none where jl >= ML), the
// lane-constant trailing coordinates xc with the innermost one set, and with HL == 1 the terms hoisted on it.  cur1: for
// HL == 2, the second-last sample index the hoisted terms were made for.  (xc and cur1 are the kernel's own locals: in a
// struct with other members they cost the HL = 2 instantiations up to 12 VGPRs.)
template <int D, int C, int K, int HL, bool IC>
__device__ __forceinline__ int render_begin_pass(const RenderArgs& a, const RenderFrame<D>& f, const RenderLane& n,
                                                 const float* __restrict__ s_ax, int pass, BlockRegs<D, C, K>& R,
                                                 float (&xc)[D], int& cur1) {
    const int jl = n.jl0 + pass * a.CL;
#pragma unroll
    for (int l = 0; l < D; ++l) xc[l] = 0.0f;
    xc[D - 1] = s_ax[f.ax_off[D - 1] + min(jl, f.ML - 1)];
    cur1 = -1;
    if (HL == 1) hoist_const<D, C, K, HL, IC>(R, xc);
    return jl;
}

// The coordinates x of the lane's sample of outer tuple o (jo: its sample index per outer axis); HL == 2 re-derives the
// hoisted terms when the second-last index changes
template <int D, int C, int K, int HL, bool IC>
__device__ __forceinline__ void render_fetch_coords(const RenderArgs& a, const RenderFrame<D>& f, const float* __restrict__ s_ax,
                                                    int o, BlockRegs<D, C, K>& R, float (&xc)[D], int& cur1, float (&x)[D],
                                                    int (&jo)[D - 1]) {
    x[D - 1] = xc[D - 1];
    if constexpr (D == 3) {
        jo[0] = o / a.m[1];
        jo[1] = o - jo[0] * a.m[1];
        x[0] = s_ax[jo[0]];
        x[1] = s_ax[f.ax_off[1] + jo[1]];
        if (HL == 2 && jo[1] != cur1) {
            xc[1] = x[1];
            hoist_const<D, C, K, HL, IC>(R, xc);
            cur1 = jo[1];
        }
    } else {
        jo[0] = o;
        x[0] = s_ax[o];
    }
}

// pixel<> as the evaluation runs it on the own block: no target, no loss, no gradient
template <int D, int C, int K, int HL, bool IC>
__device__ __forceinline__ void render_eval(const RenderArgs& a, BlockRegs<D, C, K>& R, const float (&x)[D], PixelOut<D, C, K>& po) {
    using Lt = Layout<D, C, K>;
    float t0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t0[c] = 0.0f;
    float acc[Lt::NSLOT];
#pragma unroll
    for (int j = 0; j < Lt::NSLOT; ++j) acc[j] = 0.0f;
    pixel<D, C, K, false, HL, false, IC, false>(R, a.kc, x, t0, 1.0f, acc, po);
}

// One sample into the staging buffer of the step: its values in the image's format, its kernel id
template <int D, int C, int K>
__device__ __forceinline__ void render_stage_sample(const RenderArgs& a, const RenderLane& n, const RenderWalk<D, C>& w,
                                                    const PixelOut<D, C, K>& po) {
    uint32_t* sv = w.values();
    const int si = (n.ph * a.NB + n.lb) * a.CL + n.jl0;
    if (a.fmt == SMOE_IMAGE_U8) {
#pragma unroll
        for (int c = 0; c < C; ++c) sv[si * C + c] = (uint32_t)po.kq[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) sv[si * C + c] = __float_as_uint(po.q[c]);
    }
    if (a.argmax != nullptr) {
        float best;
        uint32_t arg;
        first_max_init(best, arg, 255u);
#pragma unroll
        for (int k = 0; k < K; ++k) first_max_take(best, arg, po.wt[k], (uint32_t)k);
        w.ids()[si] = arg;
    }
}

// The runs one step of the workgroup completed, from the staging buffer to the image.  cps: components per sample (C, or 1
// for the argmax plane); ve = 1 << vs: elements per vector store (1: the plane's base is not 16-byte aligned).
template <int D, bool U8>
__device__ __forceinline__ void render_flush(const RenderArgs& a, const RenderFrame<D>& f, const uint32_t* __restrict__ st,
                                             void* __restrict__ img, int cps, int vs, int it, int pass) {
    const int ve = 1 << vs;
    const int ML = f.ML;
    const bool merge = (a.CL == ML);                       // the blocks' runs adjoin: one run per outer tuple
    const int nruns = merge ? a.RP : a.RP * a.NB;
    const int maxlen = (merge ? (f.lb_hi - f.lb_lo) * ML : a.CL) * cps;
    const int cpr = ((maxlen + ve - 1) >> vs) + 1;         // 16-byte lines a run can touch
    const long long EL = a.ext[D - 1];
    for (int w = threadIdx.x; w < nruns * cpr; w += RENDER_THREADS) {
        const int run = w / cpr;
        const int ch = w - run * cpr;
        const int r = merge ? run : run / a.NB;
        const int lbA = merge ? f.lb_lo : run - r * a.NB;
        if (lbA < f.lb_lo || lbA >= f.lb_hi) continue;
        const int o = it * a.RP + r;
        if (o >= f.MO) continue;
        long long row;
        if (D == 3) {
            const int j0 = o / a.m[1], j1 = o - j0 * a.m[1];
            const long long p0 = (long long)f.g0 * a.m[0] + j0, p1 = (long long)f.g1 * a.m[1] + j1;
            if (p0 >= a.ext[0] || p1 >= a.ext[1]) continue;
            row = p0 * a.ext[1] + p1;
        } else {
            row = (long long)f.g0 * a.m[0] + o;
            if (row >= a.ext[0]) continue;
        }
        const long long sA = (long long)(f.gl0 + lbA) * ML + (long long)pass * a.CL;    // first sample of the run on its row
        long long sE = merge ? (long long)(f.gl0 + f.lb_hi) * ML : sA + min(a.CL, ML - pass * a.CL);
        if (sE > EL) sE = EL;                                                          // positions >= extent are not written
        if (sA >= sE) continue;
        render_store_run<U8>(st, img, (row * EL + sA) * cps, (row * EL + sE) * cps, (r * a.NB + lbA) * a.CL * cps, vs, ch);
    }
}

// A step of the workgroup ends: barrier, the staged values and ids to the image, the other staging buffer for the next step.
// (The next step writes the OTHER buffer while slower lanes still read this one; that step's barrier separates these reads
// from the step after it, which writes this buffer again.)
template <int D, int C>
__device__ __forceinline__ void render_flush_step(const RenderArgs& a, const RenderFrame<D>& f, RenderWalk<D, C>& w, int it, int pass) {
    __syncthreads();
    if (a.fmt == SMOE_IMAGE_U8) render_flush<D, true>(a, f, w.values(), a.image, C, w.vs_img, it, pass);
    else render_flush<D, false>(a, f, w.values(), a.image, C, w.vs_img, it, pass);
    if (a.argmax != nullptr) render_flush<D, true>(a, f, w.ids(), a.argmax, 1, w.vs_arg, it, pass);
    w.buf ^= 1;
}

template <int D, int C, int K, int HL, bool QUANT, bool IC>
__global__ void __launch_bounds__(RENDER_THREADS) render_kernel(RenderArgs a) {
    using Lt = Layout<D, C, K>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    RenderFrame<D> f;
    if (!f.place(a)) return;

    // LDS: axis tables | block images | staging (two buffers of values + kernel ids)
    float* s_ax = lds;
    float* s_par = lds + a.off_par;
    render_load_axes<D>(a, f, [&](int, int slot, float u) { s_ax[slot] = u; });
    render_load_images<D, C, K, Lt::LP_STRIDE>(a, s_par, a.NB, [&](int lb, long long& bl) {
        bl = f.id0 + lb - a.first;                                      // index into the shard's arrays
        return lb >= f.lb_lo && lb < f.lb_hi;
    });
    __syncthreads();

    const RenderLane n = render_lane<D>(a, f);
    BlockRegs<D, C, K> R;
    R.load(s_par + n.lbc * Lt::LP_STRIDE);
    if (a.kc.qmode != 0 || a.kc.qpis != 0)
        quantize_packed<D, C, K, QUANT>(R.P, a.kc, (QUANT && a.mus_grid != nullptr) ? a.mus_grid + (size_t)(f.id0 + n.lbc - a.first) * (K * D) : nullptr);
    R.template derive<IC>(a.kc);

    RenderWalk<D, C> w;
    w.begin(a, f, lds);
    for (int pass = 0; pass < w.npass; ++pass) {
        float xc[D];
        int cur1;
        const int jl = render_begin_pass<D, C, K, HL, IC>(a, f, n, s_ax, pass, R, xc, cur1);
        const bool col_ok = n.ok && jl < f.ML;
        for (int it = 0; it < w.nit; ++it) {
            const int o = it * a.RP + n.ph;
            if (col_ok && o < f.MO) {
                float x[D];
                int jo[D - 1];
                render_fetch_coords<D, C, K, HL, IC>(a, f, s_ax, o, R, xc, cur1, x, jo);
                PixelOut<D, C, K> po;
                render_eval<D, C, K, HL, IC>(a, R, x, po);
                render_stage_sample<D, C, K>(a, n, w, po);
            }
            render_flush_step<D, C>(a, f, w, it, pass);
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

// The hoisting level a block decoder runs with where the evaluation would take `hl`
inline int render_hoisting(int D, const KernelConsts& kc, int hl) {
    if (hl > D - 1) hl = D - 1;
    if (kc.qmode != 0 && hl > 1) hl = 1;                   // as the quantised evaluation (resolve_fwd)
    return hl;
}

// What tells the two block decoders apart on the host: the LDS records of a workgroup.  The plain decoder keeps the image of
// each of its NB blocks (lines = 1, halo = 0, one table per axis); the seam-free one keeps a derived record for the blocks of
// `lines` grid lines, NB + halo of each, under a cap on their bytes, and a second table per axis.
struct RenderRecords {
    int floats;               // per record
    int lines, halo;
    int tables;               // LDS tables per axis
    size_t cap;               // bytes of records per workgroup above which NB is lowered (0: none)
};

// The launch geometry of a block decoder for checked arguments: fills the geometry fields of `a` (off_w: the float offset of
// the second tables, when there are two) and `g`.  Pure host code: smoe_render / smoe_render_blend run it in front of the
// launch, the host-only test build runs it alone.  full: the triple has the kernels of the fake-quantised graph.
inline hipError_t render_layout(int D, int C, bool full, const RenderRecords& rec, RenderArgs& a, int* off_w, int hl, int lanes,
                                RenderLayout& g) {
    if (a.kc.qmode != 0 && !full) return hipErrorNotSupported;
    hl = render_hoisting(D, a.kc, hl);
    render_geometry(D, a.m, a.grid[D - 1], lanes, hl, a);
    // fewer blocks per workgroup where their records would pass the cap; the lanes that frees go to further outer sample
    // tuples (a sample's arithmetic does not depend on the geometry)
    const int nb_plain = a.NB;
    while (rec.cap > 0 && a.NB > 1 && sizeof(float) * (size_t)rec.lines * (a.NB + rec.halo) * rec.floats > rec.cap) --a.NB;
    if (a.NB < nb_plain) {
        const long MO = (D == 3) ? (long)a.m[0] * a.m[1] : a.m[0];
        long rp = RENDER_THREADS / (a.CL * a.NB);
        if (rp > MO) rp = MO;
        if (rp > a.RP) a.RP = (int)rp;
        a.chunks = (a.grid[D - 1] + a.NB - 1) / a.NB;
    }
    long msum = 0;
    for (int l = 0; l < D; ++l) msum += a.m[l];
    if (msum * rec.tables > 32768) return hipErrorNotSupported;        // the axis tables live in LDS
    const int tab = round_up((int)msum, 4);
    if (off_w != nullptr) *off_w = tab;
    a.off_par = rec.tables * tab;
    a.off_stage = a.off_par + rec.lines * (a.NB + rec.halo) * rec.floats;
    g.hl = hl;
    g.lds_bytes = sizeof(float) * ((size_t)a.off_stage + 2u * (size_t)a.RP * a.NB * a.CL * (C + 1));
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    const long long GL = a.grid[D - 1];
    const long long line_lo = a.first / GL, line_hi = ((long long)a.first + a.nb - 1) / GL;
    a.line0 = (int)line_lo;
    g.workgroups = (line_hi - line_lo + 1) * a.chunks;
    if (g.workgroups > 0x7fffffffLL) return hipErrorInvalidValue;
    return hipSuccess;
}

// The instantiation of a block decoder family for (hoisting level, fake-quantised graph, inverse covariance); null: none.
// F::kernel<HL, QUANT, IC>() names the family's kernel; the fake-quantised ones exist for FULL triples up to HL = 1.
template <typename F, bool FULL, int HL>
auto render_kernel_at(bool q, bool ic) -> decltype(F::template kernel<HL, false, false>()) {
    if constexpr (FULL && HL <= 1) {
        if (q) return ic ? F::template kernel<HL, true, true>() : F::template kernel<HL, true, false>();
    }
    if (q) return nullptr;
    return ic ? F::template kernel<HL, false, true>() : F::template kernel<HL, false, false>();
}

template <typename F, int D, bool FULL>
auto render_kernel_for(int hl, bool q, bool ic) -> decltype(F::template kernel<0, false, false>()) {
    if (hl == 0) return render_kernel_at<F, FULL, 0>(q, ic);
    if (hl == 1) return render_kernel_at<F, FULL, 1>(q, ic);
    if constexpr (D == 3) {
        if (hl == 2) return render_kernel_at<F, FULL, 2>(q, ic);
    }
    return nullptr;
}

// The tail of a decoder's launch (the shared-kernel one included): let the kernel have its dynamic LDS, launch.
template <typename Args>
hipError_t launch_decoder(void (*kern)(Args), long long workgroups, int threads, size_t lds, const Args& a, hipStream_t st) {
    const hipError_t e = allow_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(threads), lds, st, a);
    return hipGetLastError();
}

template <int D, int C, int K>
struct RenderFamily {
    template <int HL, bool QUANT, bool IC>
    static auto kernel() -> void (*)(RenderArgs) { return &render_kernel<D, C, K, HL, QUANT, IC>; }
    static constexpr RenderRecords records() { return {Layout<D, C, K>::LP_STRIDE, 1, 0, 1, 0}; }
};

template <int D, int C, int K, bool FULL>
hipError_t render_layout(RenderArgs& a, int hl, int lanes, RenderLayout& g) {
    return render_layout(D, C, FULL, RenderFamily<D, C, K>::records(), a, nullptr, hl, lanes, g);
}

// A block decoder's launch for checked arguments: the family's instantiation (none: not supported), the geometry, the launch.
// layout(a, hl, lanes, g) is the family's render_layout / render_blend_layout; r: the RenderArgs inside a.
template <typename F, int D, bool FULL, typename Args, typename Layout_>
hipError_t launch_block_decoder(Args& a, RenderArgs& r, int hl, int lanes, hipStream_t st, Layout_ layout) {
    const bool q = r.kc.qmode != 0;
    if (q && !FULL) return hipErrorNotSupported;
    const auto kern = render_kernel_for<F, D, FULL>(render_hoisting(D, r.kc, hl), q, r.kc.inverse_cov != 0);
    if (kern == nullptr) return hipErrorNotSupported;
    RenderLayout g;
    const hipError_t e = layout(a, hl, lanes, g);
    if (e != hipSuccess) return e;
    return launch_decoder(kern, g.workgroups, RENDER_THREADS, g.lds_bytes, a, st);
}

template <int D, int C, int K, bool FULL>
hipError_t launch_render(const RenderArgs& a0, int hl, int lanes, hipStream_t st) {
    RenderArgs a = a0;
    return launch_block_decoder<RenderFamily<D, C, K>, D, FULL>(a, a, hl, lanes, st, &render_layout<D, C, K, FULL>);
}

}  // namespace smoe
#endif
