// smoe_render_view.hip.h -- viewport decoder: evaluate an axis-aligned window of a fitted block model on a ragged separable
// sample grid and store the dense image [E_0, E_1(, E_2), C] of the window (smoe_render_view, include/smoe_hip.h).
//
// Definition.  Per axis the caller gives E_l samples: a coordinate per sample in the block units of the block that owns it,
// and a start table that cuts the samples into one run per block of the view (empty runs allowed).  A sample is evaluated by
// the block that owns it on every axis exactly as render_kernel evaluates a sample of that block (same active rule, same
// fake-quantised variables, same pixel<TRAIN = false>, same hoisting level); with BLEND it is cross-faded with the
// neighbouring blocks exactly as render_blend_kernel does it.
//
// Arrangement: output tiles.  The host cuts every axis into tiles (view_layout below): at most CL samples on the innermost
// axis, a few hundred outer tuples, and never more blocks than the tile's derived records may take in LDS.  A workgroup of
// 256 lanes takes one tile.  A lane owns (innermost output column, phase): its innermost coordinate, its block on the
// innermost axis and its innermost neighbour weight are lane constants; it walks the tile's outer tuples with stride RP and
// reloads its block's derived record from LDS only when a tuple lies in another block (the hoisted constants are re-derived
// then, and with HL = 2 when the second-last coordinate changes).  The DERIVED records (BlendRec of smoe_render_blend.hip.h)
// of the blocks a tile touches -- only those with a non-empty run on every axis, plus with BLEND their neighbours -- are made
// once per workgroup by one lane per record.  A step of the workgroup completes RP rows of the tile; the output is dense, so
// a row of the tile is ONE run, which leaves through the LDS staging as 16-byte non-temporal stores on 16-byte boundaries of
// the image (render_store_run), element-wise at ragged heads and tails.
//
// Nothing a sample computes depends on the tiling: the tile only decides which lane evaluates it.
#ifndef SMOE_RENDER_VIEW_HIP_H
#define SMOE_RENDER_VIEW_HIP_H

#include <algorithm>
#include <vector>

#include "smoe_render_blend.hip.h"

namespace smoe {

// what the kernel reads of a tile on one axis
struct ViewTile {
    int s0, ns;               // first sample, samples
    int e0, ne;               // first entry (non-empty run), entries
    int r0, nr;               // first record slot of the axis' record list, slots
};

__device__ __forceinline__ ViewTile view_tile(const RenderViewArgs& v, int l, int t) {
    const int32_t* tb = v.tab;
    ViewTile x;
    x.s0 = tb[v.o_tile_s[l] + t];
    x.ns = tb[v.o_tile_s[l] + t + 1] - x.s0;
    x.e0 = tb[v.o_tile_e[l] + 2 * t];
    x.ne = tb[v.o_tile_e[l] + 2 * t + 1] - x.e0;
    const int sl0 = tb[v.o_ent_slot[l] + x.e0], sl1 = tb[v.o_ent_slot[l] + x.e0 + x.ne - 1];
    const int b0 = tb[v.o_rec_block[l] + sl0], b1 = tb[v.o_rec_block[l] + sl1];
    const bool halo = v.band[l] > 0.0f;
    x.r0 = sl0 - ((halo && b0 > 0) ? 1 : 0);
    x.nr = sl1 + ((halo && b1 < v.r.grid[l] - 1) ? 1 : 0) - x.r0 + 1;
    return x;
}

template <int D, int C, int K, int HL, bool QUANT, bool IC, bool BLEND>
__global__ void __launch_bounds__(RENDER_THREADS) render_view_kernel(RenderViewArgs v) {
    using Lt = Layout<D, C, K>;
    using Rc = BlendRec<D, C, K>;
    const RenderArgs& a = v.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;

    // the workgroup's tile per axis (innermost axis fastest)
    ViewTile T[D];
    {
        unsigned rem = blockIdx.x;
#pragma unroll
        for (int l = D - 1; l >= 0; --l) {
            const unsigned nt = (unsigned)v.ntiles[l];
            const unsigned q = rem / nt;
            T[l] = view_tile(v, l, (int)(rem - q * nt));
            rem = q;
        }
    }

    // LDS: per axis [coordinates | neighbour weights | record slot of the sample's own block] of the tile's samples and the
    // block index of the tile's record slots | derived records | staging (two buffers of values + kernel ids)
    float* s_rec = lds + a.off_par;
    int nrec = 1;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        float* s_ax = lds + v.off_ax[l];
        float* s_w = s_ax + v.TS[l];
        int* s_ri = reinterpret_cast<int*>(s_w + v.TS[l]);
        int* s_gb = s_ri + v.TS[l];
        const int32_t* es = v.tab + v.o_ent_start[l];
        for (int j = tid; j < T[l].ns; j += RENDER_THREADS) {
            const int i = T[l].s0 + j;
            int lo = T[l].e0, hi = T[l].e0 + T[l].ne - 1;          // the entry with es[e] <= i < es[e + 1]
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (es[mid] <= i) lo = mid; else hi = mid - 1;
            }
            const float u = a.ax[l][i];
            float w = 0.0f;
            if (BLEND && v.band[l] > 0.0f) {
                const float whi = fminf(fmaxf(0.5f * (1.0f + (u - v.s1[l]) / v.band[l]), 0.0f), 1.0f);
                const float wlo = fminf(fmaxf(0.5f * (1.0f + (v.s0[l] - u) / v.band[l]), 0.0f), 1.0f);
                w = (whi > 0.0f) ? whi : -wlo;
            }
            s_ax[j] = u;
            s_w[j] = w;
            s_ri[j] = v.tab[v.o_ent_slot[l] + lo] - T[l].r0;
        }
        for (int k = tid; k < T[l].nr; k += RENDER_THREADS) s_gb[k] = v.tab[v.o_rec_block[l] + T[l].r0 + k];
        nrec *= T[l].nr;
    }
    __syncthreads();
    // image-wide index of the block behind a record: records are row-major over the tile's slots per axis
    auto record_id = [&](int rec) -> long long {
        long long id = 0;
        int q = rec, sl[D];
#pragma unroll
        for (int l = D - 1; l >= 0; --l) {
            const int qq = q / T[l].nr;
            sl[l] = q - qq * T[l].nr;
            q = qq;
        }
#pragma unroll
        for (int l = 0; l < D; ++l) {
            const int* s_gb = reinterpret_cast<const int*>(lds + v.off_ax[l] + 3 * v.TS[l]);
            id = id * a.grid[l] + s_gb[sl[l]];
        }
        return id;
    };
    render_load_images<D, C, K, Rc::STRIDE>(a, s_rec, nrec, [&](int rec, long long& id) {
        id = record_id(rec);
        return true;
    });
    __syncthreads();
    // one lane per record: what every lane of render_kernel does for its block, kept for all of them
    for (int rec = tid; rec < nrec; rec += RENDER_THREADS) {
        const long long id = record_id(rec);
        BlockRegs<D, C, K> B;
        B.load(s_rec + rec * Rc::STRIDE);
        if (a.kc.qmode != 0 || a.kc.qpis != 0)
            quantize_packed<D, C, K, QUANT>(B.P, a.kc, (QUANT && a.mus_grid != nullptr) ? a.mus_grid + (size_t)id * (K * D) : nullptr);
        B.template derive<IC>(a.kc);
        store_record<D, C, K>(B, s_rec + rec * Rc::STRIDE);
    }
    __syncthreads();

    const float* s_ax0 = lds + v.off_ax[0];
    const float* s_ax1 = lds + v.off_ax[(D == 3) ? 1 : 0];
    const float* s_axl = lds + v.off_ax[D - 1];
    const int TS0 = v.TS[0], TS1 = v.TS[(D == 3) ? 1 : 0], TSL = v.TS[D - 1];
    const int NL = T[D - 1].nr, N1 = (D == 3) ? T[1].nr : 1;
    const int W = T[D - 1].ns;                             // the tile's width: the length of a row's run
    const int T1 = (D == 3) ? T[1].ns : 1;
    const int NO = T[0].ns * T1;                           // outer tuples of the tile
    const int col = tid % a.CL, ph = tid / a.CL;
    const bool col_ok = col < W && ph < a.RP;
    const int jl = min(col, W - 1);

    float xc[D];
#pragma unroll
    for (int l = 0; l < D; ++l) xc[l] = 0.0f;
    xc[D - 1] = s_axl[jl];
    const int rl = reinterpret_cast<const int*>(s_axl + 2 * TSL)[jl];
    float wn[D];                                           // weight of the neighbour per axis, sd: its side
    int sd[D];
#pragma unroll
    for (int l = 0; l < D; ++l) { wn[l] = 0.0f; sd[l] = 1; }
    if (BLEND) {
        const float sw = s_axl[TSL + jl];
        sd[D - 1] = (sw > 0.0f) ? 1 : -1;
        const int gn = reinterpret_cast<const int*>(s_axl + 3 * TSL)[rl] + sd[D - 1];
        wn[D - 1] = (gn >= 0 && gn < a.grid[D - 1]) ? fabsf(sw) : 0.0f;
    }
    const int rec_step0 = N1 * NL;

    BlockRegs<D, C, K> R;
    int cur_rec = -1, cur1 = -1;
    float t0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t0[c] = 0.0f;

    uint32_t* s_stage = reinterpret_cast<uint32_t*>(lds + a.off_stage);
    const int per = a.RP * a.CL;
    const int stg = per * (C + 1);
    const int vs_img = a.vec_img ? ((a.fmt == SMOE_IMAGE_U8) ? 4 : 2) : 0;
    const int vs_arg = a.vec_arg ? 4 : 0;
    const long long EL = a.ext[D - 1];
    const int nit = (NO + a.RP - 1) / a.RP;
    int buf = 0;
    for (int it = 0; it < nit; ++it) {
        uint32_t* sv = s_stage + buf * stg;
        uint32_t* sid = sv + per * C;
        const int o = it * a.RP + ph;
        if (col_ok && o < NO) {
            float x[D];
            x[D - 1] = xc[D - 1];
            int j0 = o, j1 = 0;
            if (D == 3) { j0 = o / T1; j1 = o - j0 * T1; }
            x[0] = s_ax0[j0];
            int rec = reinterpret_cast<const int*>(s_ax0 + 2 * TS0)[j0];
            if (D == 3) {
                x[1] = s_ax1[j1];
                rec = rec * N1 + reinterpret_cast<const int*>(s_ax1 + 2 * TS1)[j1];
            }
            rec = rec * NL + rl;
            if (rec != cur_rec) {                          // the tuple lies in another block: its record, its hoisted terms
                load_record<D, C, K>(R, s_rec + rec * Rc::STRIDE);
                cur_rec = rec;
                cur1 = -1;
                if (HL == 1) hoist_const<D, C, K, HL, IC>(R, xc);
            }
            if (D == 3 && HL == 2 && j1 != cur1) {
                xc[1] = x[1];
                hoist_const<D, C, K, HL, IC>(R, xc);
                cur1 = j1;
            }
            PixelOut<D, C, K> po;
            render_eval<D, C, K, HL, IC>(a, R, x, po);
            if constexpr (BLEND) {
                {
                    const float w0 = s_ax0[TS0 + j0];
                    sd[0] = (w0 > 0.0f) ? 1 : -1;
                    const int gn = reinterpret_cast<const int*>(s_ax0 + 3 * TS0)[reinterpret_cast<const int*>(s_ax0 + 2 * TS0)[j0]] + sd[0];
                    wn[0] = (gn >= 0 && gn < a.grid[0]) ? fabsf(w0) : 0.0f;
                }
                if (D == 3) {
                    const float w1 = s_ax1[TS1 + j1];
                    sd[1] = (w1 > 0.0f) ? 1 : -1;
                    const int gn = reinterpret_cast<const int*>(s_ax1 + 3 * TS1)[reinterpret_cast<const int*>(s_ax1 + 2 * TS1)[j1]] + sd[1];
                    wn[1] = (gn >= 0 && gn < a.grid[1]) ? fabsf(w1) : 0.0f;
                }
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
                            float Wc = 1.0f;
                            float xn[D];
                            int nrc = rec;
#pragma unroll
                            for (int l = 0; l < D; ++l) {
                                const bool nb = ((cm >> l) & 1) != 0;
                                const int step = (l == D - 1) ? 1 : ((l == 0) ? rec_step0 : NL);
                                Wc *= nb ? wn[l] : 1.0f - wn[l];
                                xn[l] = nb ? x[l] - (float)sd[l] * v.pitch[l] : x[l];
                                nrc += nb ? sd[l] * step : 0;
                            }
                            if (__ballot(Wc > 0.0f) == 0ull) continue; // wave-uniform
                            if (Wc > 0.0f) {
                                BlockRegs<D, C, K> N;
                                load_record<D, C, K>(N, s_rec + nrc * Rc::STRIDE);
                                float accn[Lt::NSLOT];
#pragma unroll
                                for (int j = 0; j < Lt::NSLOT; ++j) accn[j] = 0.0f;
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
                            po.kq[c] = floorf(fmaf(val, a.kc.inv_scale, 0.5f));
                            po.q[c] = po.kq[c] * a.kc.scale;
                        }
                    }
                }
            }
            // the sample into the staging buffer of the step: its values in the image's format, its kernel id
            const int si = ph * a.CL + col;
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
                sid[si] = arg;
            }
        }
        __syncthreads();
        // the RP rows the step completed, one run each.  (The next step writes the OTHER buffer while slower lanes still
        // read this one; that step's barrier separates these reads from the step after it, which writes this buffer again.)
        for (int plane = 0; plane < 2; ++plane) {
            if (plane == 1 && a.argmax == nullptr) break;
            const int cps = plane ? 1 : C;
            const int vs = plane ? vs_arg : vs_img;
            const int cpr = ((W * cps + (1 << vs) - 1) >> vs) + 1;     // 16-byte lines a run can touch
            for (int w = tid; w < a.RP * cpr; w += RENDER_THREADS) {
                const int r = w / cpr;
                const int ch = w - r * cpr;
                const int oo = it * a.RP + r;
                if (oo >= NO) continue;
                long long row;
                if (D == 3) {
                    const int q0 = oo / T1, q1 = oo - q0 * T1;
                    row = (long long)(T[0].s0 + q0) * a.ext[1] + (T[1].s0 + q1);
                } else {
                    row = T[0].s0 + oo;
                }
                const long long e0 = (row * EL + T[D - 1].s0) * cps;
                if (plane) render_store_run<true>(sid, a.argmax, e0, e0 + (long long)W * cps, r * a.CL * cps, vs, ch);
                else if (a.fmt == SMOE_IMAGE_U8) render_store_run<true>(sv, a.image, e0, e0 + (long long)W * cps, r * a.CL * cps, vs, ch);
                else render_store_run<false>(sv, a.image, e0, e0 + (long long)W * cps, r * a.CL * cps, vs, ch);
            }
        }
        buf ^= 1;
    }
}

constexpr size_t VIEW_RECORD_BYTES = 48u * 1024u;          // derived records of a tile, as the seam-free decoder's cap
constexpr int VIEW_MAX_TUPLES = 1024;                      // outer tuples of a tile

// The tiling and the LDS carve-up of a view for checked arguments: fills tab, the table offsets and the geometry fields of v,
// and g.  start[l]: the caller's start table of view_blocks[l] + 1 entries; first[l]: the view's first block on the axis.
// hipErrorNotSupported: the records of the smallest tile (one block per axis, three with a blend on the axis) pass the cap,
// the launch would need 2^31 workgroups or more, or the tile does not fit 160 KB of LDS.
inline hipError_t view_layout(int D, int C, int rec_floats, const int32_t* const start[3], const int32_t first[3],
                              const int32_t blocks[3], RenderViewArgs& v, ViewPlan& plan, RenderLayout& g) {
    RenderArgs& a = v.r;
    std::vector<int32_t> ent_start[3], ent_block[3], ent_slot[3], rec_block[3], tile_s[3], tile_e[3];
    for (int l = 0; l < D; ++l) {
        const bool halo = v.band[l] > 0.0f;
        for (int j = 0; j < blocks[l]; ++j) {
            if (start[l][j + 1] == start[l][j]) continue;
            const int b = first[l] + j;
            ent_start[l].push_back(start[l][j]);
            ent_block[l].push_back(b);
            for (int nb = halo ? b - 1 : b; nb <= (halo ? b + 1 : b); ++nb) {
                if (nb < 0 || nb >= a.grid[l]) continue;
                if (rec_block[l].empty() || rec_block[l].back() < nb) rec_block[l].push_back(nb);
            }
        }
        ent_start[l].push_back(start[l][blocks[l]]);
        size_t s = 0;
        for (size_t e = 0; e < ent_block[l].size(); ++e) {
            while (rec_block[l][s] != ent_block[l][e]) ++s;
            ent_slot[l].push_back((int32_t)s);
        }
    }
    // record slots per axis and tile under the cap: from one own block per axis (with a blend on the axis: and its two
    // neighbours), the axis whose own blocks cover the smallest share of its target grows -- 256 samples and one more block
    // on the innermost axis, 16 samples (at most 8 blocks) on an outer axis
    const long long cap_total = (long long)(VIEW_RECORD_BYTES / (sizeof(float) * rec_floats));
    int cap[3] = {1, 1, 1};
    long long own[3] = {1, 1, 1}, lim[3] = {1, 1, 1}, per_entry[3] = {1, 1, 1}, tgt[3] = {16, 16, 16}, halo2[3] = {0, 0, 0};
    long long prod = 1;
    for (int l = 0; l < D; ++l) {
        const long long ne = (long long)ent_block[l].size();
        halo2[l] = (v.band[l] > 0.0f) ? 2 : 0;
        per_entry[l] = (a.ext[l] + ne - 1) / ne;
        if (l == D - 1) tgt[l] = RENDER_THREADS;
        lim[l] = (l == D - 1) ? std::min<long long>(ne, (RENDER_THREADS + per_entry[l] - 1) / per_entry[l] + 1) : std::min<long long>(ne, 8);
        prod *= 1 + halo2[l];
    }
    if (prod > cap_total) return hipErrorNotSupported;
    for (;;) {
        int best = -1;
        for (int l = 0; l < D; ++l) {
            if (own[l] >= lim[l] || prod / (own[l] + halo2[l]) * (own[l] + 1 + halo2[l]) > cap_total) continue;
            if (best < 0 || own[l] * per_entry[l] * tgt[best] <= own[best] * per_entry[best] * tgt[l]) best = l;
        }
        if (best < 0) break;
        prod = prod / (own[best] + halo2[best]) * (own[best] + 1 + halo2[best]);
        ++own[best];
    }
    for (int l = 0; l < D; ++l) cap[l] = (int)(own[l] + halo2[l]);
    // lanes: CL columns of the tile, RP rows per step.  Equal tiles across the extent; no wider than the samples the innermost
    // record slots of a tile are expected to own (a thumbnail has about one sample per block)
    const long long EL = a.ext[D - 1];
    {
        const long long own_last = own[D - 1];
        const long long per_entry_last = per_entry[D - 1];
        const long long width = std::min<long long>(RENDER_THREADS, std::max<long long>(1, own_last * per_entry_last));
        const long long cols_ = (EL + width - 1) / width;
        a.CL = (int)((EL + cols_ - 1) / cols_);
        a.RP = RENDER_THREADS / a.CL;
        a.NB = 1;
    }
    const long long cols = (EL + a.CL - 1) / a.CL;
    // samples per axis and tile: enough workgroups to fill the device, enough tuples to pay for a tile's records
    long long outer = 1;
    for (int l = 0; l < D - 1; ++l) outer *= a.ext[l];
    long long tuples = outer * cols / 1024;
    const long long tmin = 4LL * a.RP, tmax = std::max<long long>(tmin, std::min<long long>(64LL * a.RP, VIEW_MAX_TUPLES));
    tuples = std::max(tmin, std::min(tuples, tmax));
    long long ts[3] = {1, 1, 1};
    ts[D - 1] = a.CL;
    if (D == 3) {
        ts[1] = std::min<long long>(a.ext[1], tuples);
        ts[0] = std::max<long long>(1, tuples / ts[1]);
    } else {
        ts[0] = tuples;
    }
    int nr_max[3] = {1, 1, 1};
    long long wgs = 1;
    for (int l = 0; l < D; ++l) {
        const bool halo = v.band[l] > 0.0f;
        const long long E = a.ext[l];
        const int ne = (int)ent_block[l].size();
        long long s = 0;
        int e = 0;
        int ts_max = 1;
        while (s < E) {
            while (ent_start[l][e + 1] <= s) ++e;
            long long end = std::min(E, s + ts[l]);
            int hi = e;
            while (hi + 1 < ne && ent_start[l][hi + 1] < end) ++hi;
            auto slots = [&](int last) {
                const int lo_h = (halo && ent_block[l][e] > 0) ? 1 : 0, hi_h = (halo && ent_block[l][last] < a.grid[l] - 1) ? 1 : 0;
                return ent_slot[l][last] + hi_h - (ent_slot[l][e] - lo_h) + 1;
            };
            while (slots(hi) > cap[l]) { --hi; end = ent_start[l][hi + 1]; }
            tile_s[l].push_back((int32_t)s);
            tile_e[l].push_back(e);
            tile_e[l].push_back(hi + 1);
            nr_max[l] = std::max(nr_max[l], slots(hi));
            ts_max = std::max<int>(ts_max, (int)(end - s));
            s = end;
        }
        tile_s[l].push_back((int32_t)E);
        v.ntiles[l] = (int)tile_s[l].size() - 1;
        v.TS[l] = ts_max;
        wgs *= v.ntiles[l];
        if (wgs > 0x7fffffffLL) return hipErrorNotSupported;
    }
    for (int l = D; l < 3; ++l) { v.ntiles[l] = 1; v.TS[l] = 0; }
    // the device table
    plan.tab.clear();
    auto put = [&](const std::vector<int32_t>& x) {
        const int o = (int)plan.tab.size();
        plan.tab.insert(plan.tab.end(), x.begin(), x.end());
        return o;
    };
    for (int l = 0; l < D; ++l) {
        v.o_ent_start[l] = put(ent_start[l]);
        v.o_ent_slot[l] = put(ent_slot[l]);
        v.o_rec_block[l] = put(rec_block[l]);
        v.o_tile_s[l] = put(tile_s[l]);
        v.o_tile_e[l] = put(tile_e[l]);
    }
    // LDS
    size_t off = 0, nrec = 1;
    for (int l = 0; l < D; ++l) {
        v.off_ax[l] = (int)off;
        off += round_up(3 * v.TS[l] + nr_max[l], 4);
        nrec *= (size_t)nr_max[l];
    }
    a.off_par = (int)off;
    a.off_stage = a.off_par + (int)(nrec * rec_floats);
    g.lds_bytes = sizeof(float) * ((size_t)a.off_stage + 2u * (size_t)a.RP * a.CL * (C + 1));
    if (g.lds_bytes > 160u * 1024u) return hipErrorNotSupported;
    g.workgroups = wgs;
    return hipSuccess;
}

template <int D, int C, int K, bool BLEND>
struct RenderViewFamily {
    template <int HL, bool QUANT, bool IC>
    static auto kernel() -> void (*)(RenderViewArgs) { return &render_view_kernel<D, C, K, HL, QUANT, IC, BLEND>; }
};

template <int D, int C, int K, bool FULL>
hipError_t render_view_layout(RenderViewArgs& v, const ViewHost& hst, ViewPlan& plan, int hl, RenderLayout& g) {
    if (v.r.kc.qmode != 0 && !FULL) return hipErrorNotSupported;
    g.hl = render_hoisting(D, v.r.kc, hl);
    return view_layout(D, C, BlendRec<D, C, K>::STRIDE, hst.start, hst.first, hst.blocks, v, plan, g);
}

// The kernel of a planned view (v.tab on the device, geometry filled by render_view_layout): the launch alone.
template <int D, int C, int K, bool FULL>
hipError_t launch_render_view(const RenderViewArgs& v, const RenderLayout& g, hipStream_t st) {
    const bool q = v.r.kc.qmode != 0;
    if (q && !FULL) return hipErrorNotSupported;
    bool blend = false;
    for (int l = 0; l < D; ++l) blend = blend || v.band[l] > 0.0f;
    const auto kern = blend ? render_kernel_for<RenderViewFamily<D, C, K, true>, D, FULL>(g.hl, q, v.r.kc.inverse_cov != 0)
                            : render_kernel_for<RenderViewFamily<D, C, K, false>, D, FULL>(g.hl, q, v.r.kc.inverse_cov != 0);
    if (kern == nullptr) return hipErrorNotSupported;
    return launch_decoder(kern, g.workgroups, RENDER_THREADS, g.lds_bytes, v, st);
}

}  // namespace smoe
#endif
