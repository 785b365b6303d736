// smoe_sample.hip.h -- point decoder: evaluate a fitted block model at a list of arbitrary positions and store the dense
// results [N, C] (smoe_sample, include/smoe_hip.h).
//
// Definition.  A point is D float32 numbers in source pixels, in the image's axis order; pixel q covers [q, q + 1).  A point
// with a NaN, x < 0 or x >= length[l] on any axis is OUTSIDE: values 0, argmax 255, block -1, nothing else computed.  Otherwise
// per axis (n = block_shape[l]) its block is the integer g with g n <= x < (g + 1) n -- floorf(x / n), corrected by +-1 against
// the products g n and (g + 1) n, which are exact in fp32 (grid n <= 2^24) -- and its block-unit coordinate is
// u = ((x - g n) - 0.5f) / (n - 1): an exact subtraction, one rounded subtraction, one correctly rounded division (0 for n == 1)
// (sample_resolve below; blocks.point_blocks is the same statement in numpy).  The own block (image-wide index row-major over
// the grid) is evaluated at u exactly as render_kernel evaluates a sample of that block for prod(grid) blocks; with BLEND it is
// cross-faded with the neighbouring blocks exactly as render_blend_kernel / render_view_kernel do it.  argmax is the own
// block's.  Nothing a point computes depends on the other points, on its place in the list or on how the launch is cut.
//
// Arrangement: that of the point frame (point_box ... point_store_plane below), of which smoe_sample_grad.hip.h is built;
// this kernel spells most of it out in its own text (see the frame's comment for why).  A workgroup of 256 lanes takes
// PPL * 256 consecutive points (PPL = SAMPLE_PPL here): lane t takes the PPL points from t * PPL on, so a lane's points and
// those of its neighbours are neighbours in the list, a row-major warp keeps a wavefront inside one or two blocks and a lane
// mostly inside one.  The workgroup first resolves its points and takes the per-axis minimum and maximum of their block
// indices (with BLEND widened by one inside the grid).
//  * Staged path: the box has no more blocks than the record budget (s.rec_cap).  One lane per block of the box derives its
//    record (sample_derive: what every lane of render_kernel does for its block) and keeps it in LDS (store_record); a lane
//    reads a record (load_record) when its point's block differs from the one it holds, and a neighbour's when it needs one.
//  * Direct path: otherwise.  Every lane derives the record of its point's block -- and of a neighbour it needs -- from global
//    memory in registers, again with sample_derive, when the block differs from the one it holds.
// Both paths run the same device functions on the same inputs, so they give the same bits.  A point is located (block,
// coordinates, record), with BLEND the neighbour window of every axis and the geometry of every corner of the cross-fade
// are formed, and the planes are stored: the workgroup's results are turned through LDS and leave, after one barrier, as 16-byte non-temporal stores
// where the plane's base is 16-byte aligned, element-wise at the ragged head and tail (render_store_run) -- the output is
// dense, so a workgroup's points are one run per plane.  What a point computes is the kernel's: here the hoisted terms are
// re-made for every point from its own trailing coordinates (hoist_const), the same fused multiply-adds in the same order as
// in render_kernel, where those coordinates are lane constants.
#ifndef SMOE_SAMPLE_HIP_H
#define SMOE_SAMPLE_HIP_H

#include "smoe_render_view.hip.h"

namespace smoe {

constexpr int SAMPLE_PPL = 4;                               // points per lane
// Staged records of a workgroup, at most.  A quarter of the viewport decoder's 48 KB: beside the 20 KB of staging (C = 3) that
// leaves the register file, not LDS, to set the occupancy, and a box that needs more is cheaper on the direct path anyway,
// whose lanes derive one block per run of points (measured).
constexpr size_t SAMPLE_RECORD_BYTES = 12u * 1024u;

// the block index g and the block-unit coordinate u of position x on an axis of `len` pixels in blocks of n; false: outside
__device__ __forceinline__ bool sample_resolve(float x, int n, float len, int& g, float& u) {
    g = 0;
    u = 0.0f;
    if (!(x >= 0.0f) || x >= len) return false;
    g = (int)floorf(__fdiv_rn(x, (float)n));
    if ((float)(g * n) > x) --g;
    else if ((float)((g + 1) * n) <= x) ++g;
    const float t = x - (float)(g * n);
    u = (n > 1) ? __fdiv_rn(t - 0.5f, (float)(n - 1)) : 0.0f;
    return true;
}

// A value before the lattice onto the 8-bit lattice: its index (the value is index * kc.scale).  The one rounding of the
// point decoders' own results: sample_kernel's cross-fade and sample_area_kernel's mean (smoe_sample_area.hip.h).
__device__ __forceinline__ float lattice_index(const KernelConsts& kc, float v) { return floorf(fmaf(v, kc.inv_scale, 0.5f)); }

// What every lane of render_kernel does for its block, from global memory: the block image (packed parameters, `active`
// flags), the fake-quantised variables, the derived constants.  id: image-wide block index.
template <int D, int C, int K, bool QUANT, bool IC>
__device__ __forceinline__ void sample_derive(const RenderArgs& a, long long id, BlockRegs<D, C, K>& B) {
    using Lt = Layout<D, C, K>;
    const uint32_t act = (a.active == nullptr) ? 0xffffffffu : a.active[id];
    // (two short loops, not one over the LP_STRIDE cells: the long one is unrolled too late for K = 8 and B stays in scratch)
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 0; o < Lt::PK; ++o) {
            int tensor, kern;
            long off;
            decode_slot<D, C, K>(k * Lt::PK + o, (int)id, tensor, off, kern);
            B.P[k * Lt::PK + o] = pick(a.p, tensor)[off];
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) B.P[Lt::LP_ACT + k] = ((act >> k) & 1u) ? 1.0f : 0.0f;
#pragma unroll
    for (int j = Lt::LP_ACT + K; j < Lt::LP_STRIDE; ++j) B.P[j] = 0.0f;
    if (a.kc.qmode != 0 || a.kc.qpis != 0)
        quantize_packed<D, C, K, QUANT>(B.P, a.kc, (QUANT && a.mus_grid != nullptr) ? a.mus_grid + (size_t)id * (K * D) : nullptr);
    B.template derive<IC>(a.kc);
}

// The point decoders' frame: what a point decoder does around the evaluation of a point, and nothing of the evaluation.  A
// workgroup of 256 lanes takes PPL * 256 consecutive points [p0, pe), lane t the PPL points from t * PPL on.  LDS: box (per
// axis minimum, maximum of the block indices) | derived records (s_rec, from r.off_par) | the kernel's own staging (from
// r.off_stage).  The pieces are free functions over the kernel's own locals p0, pe, lo, nbx, staged and s_rec.
// sample_grad_kernel is built from all of them; the two lines that give p0 / pe and the staging loop between point_box and
// the prologue's last barrier stand in its text, word for word as in sample_kernel.
// sample_kernel (below) uses point_window and point_fetch and keeps the rest in its own text: with these two its
// instruction stream is the one it had before the frame in every instantiation (in a quarter of them up to four integer
// additions have their operands swapped).  Any of point_box, point_locate, point_corner or point_store_plane in place of
// its own lines leaves the compiler the same instructions in another order after inlining, and with that another register
// allocation and schedule: of the arrangements tried, each either cost some instantiations a wave per SIMD or 0.5 ... 1.4 %
// of the kernel's time (profiles/render/point_frame_ab.txt).

// The prologue up to the box, with two barriers: every lane of the workgroup runs it, once, before anything else.  The
// workgroup resolves its points and takes the box of their blocks: first block lo and blocks nbx per axis, with BLEND widened
// by one inside the grid.  Returns the blocks of the box; where they are no more than the record budget (s.rec_cap) the
// kernel has one lane per block derive its record into LDS (staged, workgroup-uniform) and closes with a third barrier.
template <int D, int PPL, bool BLEND>
__device__ __forceinline__ long long point_box(const SampleArgs& s, float* lds, long long p0, long long pe, int (&lo)[D],
                                               int (&nbx)[D]) {
    const RenderArgs& a = s.r;
    const int tid = threadIdx.x;
    int* s_box = reinterpret_cast<int*>(lds);
    if (tid < D) { s_box[2 * tid] = 0x7fffffff; s_box[2 * tid + 1] = -1; }
    __syncthreads();
    for (int j = 0; j < PPL; ++j) {
        const long long i = p0 + tid * PPL + j;
        if (i >= pe) break;
        int g[D];
        bool in = true;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            float u;
            in = sample_resolve(s.points[i * D + l], s.n[l], s.length[l], g[l], u) && in;
        }
        if (in) {
#pragma unroll
            for (int l = 0; l < D; ++l) {                  // (a stale read only costs an atomic that changes nothing)
                if (g[l] < s_box[2 * l]) atomicMin(&s_box[2 * l], g[l]);
                if (g[l] > s_box[2 * l + 1]) atomicMax(&s_box[2 * l + 1], g[l]);
            }
        }
    }
    __syncthreads();
    long long nrec = 1;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        int b0 = s_box[2 * l], b1 = s_box[2 * l + 1];
        if (BLEND && s.band[l] > 0.0f) { b0 = max(b0 - 1, 0); b1 = min(b1 + 1, a.grid[l] - 1); }
        lo[l] = b0;
        nbx[l] = (b1 >= b0) ? b1 - b0 + 1 : 0;
        nrec *= nbx[l];
    }
    return nrec;
}

// the record of block (id image-wide, rec in the box) into registers
template <int D, int C, int K, bool QUANT, bool IC>
__device__ __forceinline__ void point_fetch(const SampleArgs& s, bool staged, const float* s_rec, BlockRegs<D, C, K>& B,
                                            long long id, int rec) {
    if (staged) load_record<D, C, K>(B, s_rec + rec * BlendRec<D, C, K>::STRIDE);
    else sample_derive<D, C, K, QUANT, IC>(s.r, id, B);
}

// The position pt in source pixels: false where it is outside (id -1).  Otherwise its block g, its block-unit coordinates x,
// the block's image-wide index id and its record's index rec in the box.
template <int D>
__device__ __forceinline__ bool point_locate_at(const SampleArgs& s, const int (&lo)[D], const int (&nbx)[D], const float (&pt)[D],
                                                int (&g)[D], float (&x)[D], long long& id, int& rec) {
    bool in = true;
#pragma unroll
    for (int l = 0; l < D; ++l) in = sample_resolve(pt[l], s.n[l], s.length[l], g[l], x[l]) && in;
    id = -1;
    rec = 0;
    if (in) {
        id = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            id = id * s.r.grid[l] + g[l];
            rec = rec * nbx[l] + (g[l] - lo[l]);
        }
    }
    return in;
}

// point i of the list
template <int D>
__device__ __forceinline__ bool point_locate(const SampleArgs& s, const int (&lo)[D], const int (&nbx)[D], long long i,
                                             int (&g)[D], float (&x)[D], long long& id, int& rec) {
    float pt[D];
#pragma unroll
    for (int l = 0; l < D; ++l) pt[l] = s.points[i * D + l];
    return point_locate_at<D>(s, lo, nbx, pt, g, x, id, rec);
}

// The neighbour window of axis l at coordinate x in block g: the signed weight w (> 0: towards the high neighbour), the
// neighbour's side sd and its weight wn = |w|, 0 where the neighbour is outside the grid.
__device__ __forceinline__ float point_window(const SampleArgs& s, int l, float x, int g, int& sd, float& wn) {
    float w = 0.0f;
    if (s.band[l] > 0.0f) {
        const float whi = fminf(fmaxf(0.5f * (1.0f + (x - s.s1[l]) / s.band[l]), 0.0f), 1.0f);
        const float wlo = fminf(fmaxf(0.5f * (1.0f + (s.s0[l] - x) / s.band[l]), 0.0f), 1.0f);
        w = (whi > 0.0f) ? whi : -wlo;
    }
    sd = (w > 0.0f) ? 1 : -1;
    const int gn = g + sd;
    wn = (gn >= 0 && gn < s.r.grid[l]) ? fabsf(w) : 0.0f;
    return w;
}

// Corner cm of a point (bit l = the neighbour on axis l): its weight, the point's coordinates xn in that block, the block's
// image-wide index nid and its record nrc.  (A neighbour outside the grid has weight 0: nid / nrc are not to be used.)
template <int D>
__device__ __forceinline__ float point_corner(const SampleArgs& s, const int (&lo)[D], const int (&nbx)[D], int cm,
                                              const int (&g)[D], const float (&x)[D], const int (&sd)[D], const float (&wn)[D],
                                              float (&xn)[D], long long& nid, int& nrc) {
    float Wc = 1.0f;
    nid = 0;
    nrc = 0;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        const bool nb = ((cm >> l) & 1) != 0;
        const int gg = g[l] + (nb ? sd[l] : 0);
        Wc *= nb ? wn[l] : 1.0f - wn[l];
        xn[l] = nb ? x[l] - (float)sd[l] * s.pitch[l] : x[l];
        nid = nid * s.r.grid[l] + gg;
        nrc = nrc * nbx[l] + (gg - lo[l]);
    }
    return Wc;
}

// The workgroup's run [p0, pe) of one plane from its staging st (a dword per value, cps values per point) to the dense
// output: vs = log2 of the values per 16-byte line where the plane's base is 16-byte aligned, else 0; u8: bytes, not dwords.
template <int PPL>
__device__ __forceinline__ void point_store_plane(long long p0, long long pe, const uint32_t* st, void* dst, int cps, int vs,
                                                  bool u8) {
    const int cpr = ((PPL * RENDER_THREADS * cps + (1 << vs) - 1) >> vs) + 1;      // 16-byte lines the run can touch
    const long long e0 = p0 * cps, e1 = pe * cps;
    for (int ch = threadIdx.x; ch < cpr; ch += RENDER_THREADS) {
        if (u8) render_store_run<true>(st, dst, e0, e1, 0, vs, ch);
        else render_store_run<false>(st, dst, e0, e1, 0, vs, ch);
    }
}

template <int D, int C, int K, int HL, bool QUANT, bool IC, bool BLEND>
__global__ void __launch_bounds__(RENDER_THREADS) sample_kernel(SampleArgs s) {
    using Lt = Layout<D, C, K>;
    const RenderArgs& a = s.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * (SAMPLE_PPL * RENDER_THREADS);    // the workgroup's first point
    const long long pe = (s.num_points - p0 < SAMPLE_PPL * RENDER_THREADS) ? s.num_points : p0 + SAMPLE_PPL * RENDER_THREADS;

    // LDS: box (per axis minimum, maximum of the block indices) | derived records | staging (values, kernel ids, block indices)
    int* s_box = reinterpret_cast<int*>(lds);
    float* s_rec = lds + a.off_par;
    if (tid < D) { s_box[2 * tid] = 0x7fffffff; s_box[2 * tid + 1] = -1; }
    __syncthreads();
    for (int j = 0; j < SAMPLE_PPL; ++j) {
        const long long i = p0 + tid * SAMPLE_PPL + j;
        if (i >= pe) break;
        int g[D];
        bool in = true;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            float u;
            in = sample_resolve(s.points[i * D + l], s.n[l], s.length[l], g[l], u) && in;
        }
        if (in) {
#pragma unroll
            for (int l = 0; l < D; ++l) {                  // (a stale read only costs an atomic that changes nothing)
                if (g[l] < s_box[2 * l]) atomicMin(&s_box[2 * l], g[l]);
                if (g[l] > s_box[2 * l + 1]) atomicMax(&s_box[2 * l + 1], g[l]);
            }
        }
    }
    __syncthreads();
    int lo[D], nbx[D];                                     // the box: first block and blocks per axis
    long long nrec = 1;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        int b0 = s_box[2 * l], b1 = s_box[2 * l + 1];
        if (BLEND && s.band[l] > 0.0f) { b0 = max(b0 - 1, 0); b1 = min(b1 + 1, a.grid[l] - 1); }
        lo[l] = b0;
        nbx[l] = (b1 >= b0) ? b1 - b0 + 1 : 0;
        nrec *= nbx[l];
    }
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

    // the record of block (id image-wide, rec in the box) into registers (a lambda, as before the frame: with point_fetch
    // called directly at its two sites the cross-fade instantiations of triple 3,1,1 lose a wave per SIMD)
    auto fetch = [&](BlockRegs<D, C, K>& B, long long id, int rec) {
        point_fetch<D, C, K, QUANT, IC>(s, staged, s_rec, B, id, rec);
    };

    BlockRegs<D, C, K> R;
    long long cur_id = -1;
    float t0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t0[c] = 0.0f;

    // staging: the values, the kernel ids and the block indices of the workgroup's points
    constexpr int per = SAMPLE_PPL * RENDER_THREADS;
    uint32_t* sv = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    uint32_t* sid = sv + per * C;
    uint32_t* sbk = sid + per;
#pragma unroll 1
    for (int j = 0; j < SAMPLE_PPL; ++j) {
        const int si = tid * SAMPLE_PPL + j;               // the lane's points are neighbours: mostly one block, one record
        const long long i = p0 + si;
        if (i < pe) {
            float x[D];
            int g[D];
            bool in = true;
#pragma unroll
            for (int l = 0; l < D; ++l) in = sample_resolve(s.points[i * D + l], s.n[l], s.length[l], g[l], x[l]) && in;
            PixelOut<D, C, K> po;
            uint32_t arg = 255u;
            long long id = -1;
            if (in) {
                int rec = 0;
                id = 0;
#pragma unroll
                for (int l = 0; l < D; ++l) {
                    id = id * a.grid[l] + g[l];
                    rec = rec * nbx[l] + (g[l] - lo[l]);
                }
                if (id != cur_id) {                        // the point lies in another block: its record
                    fetch(R, id, rec);
                    cur_id = id;
                }
                if (HL > 0) hoist_const<D, C, K, HL, IC>(R, x);
                render_eval<D, C, K, HL, IC>(a, R, x, po);
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
                            float Wc = 1.0f;
                            float xn[D];
                            int nrc = 0;
                            long long nid = 0;
#pragma unroll
                            for (int l = 0; l < D; ++l) {
                                const bool nb = ((cm >> l) & 1) != 0;
                                const int gg = g[l] + (nb ? sd[l] : 0);
                                Wc *= nb ? wn[l] : 1.0f - wn[l];
                                xn[l] = nb ? x[l] - (float)sd[l] * s.pitch[l] : x[l];
                                nid = nid * a.grid[l] + gg;
                                nrc = nrc * nbx[l] + (gg - lo[l]);
                            }
                            if (Wc > 0.0f) {               // (a neighbour outside the grid has weight 0: nid / nrc are not used)
                                BlockRegs<D, C, K> N;
                                fetch(N, nid, nrc);
                                float accn[Lt::NSLOT];
#pragma unroll
                                for (int jj = 0; jj < Lt::NSLOT; ++jj) accn[jj] = 0.0f;
                                PixelOut<D, C, K> pn;
                                pixel<D, C, K, false, 0, false, IC, false>(N, a.kc, xn, t0, 1.0f, accn, pn);
                                if (has_influence<K>(pn.wt)) {
                                    float yn[C];
                                    blend_y<D, C, K, 0>(N, xn, pn.wt, yn);
                                    den += Wc;
#pragma unroll
                                    for (int c = 0; c < C; ++c)
                                        num[c] = fmaf(Wc, __builtin_amdgcn_fmed3f(yn[c], 0.0f, a.kc.nudged_max), num[c]);
                                }
                            }
                        }
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float val = (den > 0.0f) ? num[c] / den : 0.0f;
                            po.kq[c] = lattice_index(a.kc, val);
                            po.q[c] = po.kq[c] * a.kc.scale;
                        }
                    }
                }
                float best;
                first_max_init(best, arg, 255u);
#pragma unroll
                for (int k = 0; k < K; ++k) first_max_take(best, arg, po.wt[k], (uint32_t)k);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) { po.kq[c] = 0.0f; po.q[c] = 0.0f; }
            }
            // the point into the staging buffer of the step: its values in the output's format, its kernel id, its block
            if (a.fmt == SMOE_IMAGE_U8) {
#pragma unroll
                for (int c = 0; c < C; ++c) sv[si * C + c] = (uint32_t)po.kq[c];
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) sv[si * C + c] = __float_as_uint(po.q[c]);
            }
            sid[si] = arg;
            sbk[si] = (uint32_t)(int)id;
        }
    }
    __syncthreads();
    // the workgroup's run of every plane
    const int vs_img = a.vec_img ? ((a.fmt == SMOE_IMAGE_U8) ? 4 : 2) : 0;
    const int vs_arg = a.vec_arg ? 4 : 0;
    const int vs_blk = s.vec_blk ? 2 : 0;
    for (int plane = 0; plane < 3; ++plane) {
        if (plane == 1 && a.argmax == nullptr) continue;
        if (plane == 2 && s.block == nullptr) continue;
        const int cps = (plane == 0) ? C : 1;
        const int vs = (plane == 0) ? vs_img : ((plane == 1) ? vs_arg : vs_blk);
        const int cpr = ((per * cps + (1 << vs) - 1) >> vs) + 1;           // 16-byte lines the run can touch
        const long long e0 = p0 * cps, e1 = pe * cps;
        for (int ch = tid; ch < cpr; ch += RENDER_THREADS) {
            if (plane == 2) render_store_run<false>(sbk, s.block, e0, e1, 0, vs, ch);
            else if (plane == 1) render_store_run<true>(sid, a.argmax, e0, e1, 0, vs, ch);
            else if (a.fmt == SMOE_IMAGE_U8) render_store_run<true>(sv, a.image, e0, e1, 0, vs, ch);
            else render_store_run<false>(sv, a.image, e0, e1, 0, vs, ch);
        }
    }
}

// The launch geometry and the LDS carve-up of a point decoder for checked arguments: pure host code.  stage_dwords: what a
// point stages, ppl: the points per lane.  records: the cap on the staged records of a workgroup the caller asks for (< 0:
// none; 0: always the direct path).  The budget: at most SAMPLE_RECORD_BYTES of records -- where not even the smallest set a
// point needs (its block, with a blend the 3^d around it) fits, nothing is staged --, never more records than the grid has
// blocks, 160 KB of LDS in all.
inline hipError_t point_layout(int D, int stage_dwords, int ppl, int rec_floats, long long records, SampleArgs& s, RenderLayout& g) {
    RenderArgs& a = s.r;
    long long cap = (long long)(SAMPLE_RECORD_BYTES / (sizeof(float) * rec_floats));
    long long least = 1, total = 1;
    for (int l = 0; l < D; ++l) {
        least *= (s.band[l] > 0.0f) ? std::min(3, a.grid[l]) : 1;
        total *= a.grid[l];
    }
    if (least > cap) cap = 0;
    if (cap > total) cap = total;
    if (records >= 0 && records < cap) cap = records;
    s.rec_cap = (int)cap;
    a.off_par = round_up(2 * D, 4);
    a.off_stage = a.off_par + (int)cap * rec_floats;
    const long long per = (long long)ppl * RENDER_THREADS;
    g.lds_bytes = sizeof(float) * ((size_t)a.off_stage + (size_t)per * stage_dwords);
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    g.workgroups = (s.num_points + per - 1) / per;
    if (g.workgroups > 0x7fffffffLL) return hipErrorNotSupported;
    return hipSuccess;
}

template <int D, int C, int K, bool BLEND>
struct SampleFamily {
    template <int HL, bool QUANT, bool IC>
    static auto kernel() -> void (*)(SampleArgs) { return &sample_kernel<D, C, K, HL, QUANT, IC, BLEND>; }
};

template <int D, int C, int K, bool FULL>
hipError_t sample_layout(SampleArgs& s, int hl, long long records, RenderLayout& g) {
    if (s.r.kc.qmode != 0 && !FULL) return hipErrorNotSupported;
    g.hl = render_hoisting(D, s.r.kc, hl);
    return point_layout(D, C + 2, SAMPLE_PPL, BlendRec<D, C, K>::STRIDE, records, s, g);   // a point stages C values, id, block
}

// The kernel of a planned call (geometry filled by sample_layout): the launch alone.
template <int D, int C, int K, bool FULL>
hipError_t launch_sample(const SampleArgs& s, const RenderLayout& g, hipStream_t st) {
    const bool q = s.r.kc.qmode != 0;
    if (q && !FULL) return hipErrorNotSupported;
    bool blend = false;
    for (int l = 0; l < D; ++l) blend = blend || s.band[l] > 0.0f;
    const auto kern = blend ? render_kernel_for<SampleFamily<D, C, K, true>, D, FULL>(g.hl, q, s.r.kc.inverse_cov != 0)
                            : render_kernel_for<SampleFamily<D, C, K, false>, D, FULL>(g.hl, q, s.r.kc.inverse_cov != 0);
    if (kern == nullptr) return hipErrorNotSupported;
    return launch_decoder(kern, g.workgroups, RENDER_THREADS, g.lds_bytes, s, st);
}

}  // namespace smoe
#endif
