// view_args_driver.cpp -- the argument checks and the host plan of smoe_render_view (csrc/smoe_capi.hip,
// csrc/smoe_render_view.hip.h) on a box WITHOUT a GPU, under AddressSanitizer + UndefinedBehaviorSanitizer: linked with the
// host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1: handles without a device, launches compiled out), so every call
// runs up to the point where it would launch -- the tiling, the device table and its copy into the handle's workspace
// included.  The plan itself (Variant::render_view_layout) is also run directly and its table checked: the tiles partition
// every axis, no tile exceeds the LDS tables sized for it, every sample has its entry, every neighbour its record slot.
// Built by `make -C steered_mixture_of_experts_amd/csrc hostcheck_view`.  Test infrastructure: tests/test_view_render_host.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "smoe_device.h"
#include "smoe_hip.h"

static int g_checks = 0, g_fail = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, smoe_last_error()); } \
    } while (0)

static smoe_config config(int dim, int ch, int k, int b0, int b1, int b2) {
    smoe_config c;
    std::memset(&c, 0, sizeof c);
    c.abi_version = SMOE_ABI_VERSION;
    c.dim = dim; c.block_shape[0] = b0; c.block_shape[1] = b1; c.block_shape[2] = b2;
    c.channels = ch; c.kernels = k; c.precision = 8; c.margin = 0.5f;
    c.use_determinant = 1; c.train_pis = c.train_gammas = c.train_musx = 1;
    c.lr_expert = 1e-3f; c.lr_pis = 1e-5f; c.lr_steer = 1.0f; c.beta1 = 0.9f; c.beta2 = 0.999f; c.adam_eps = 1e-8f;
    c.start_pis = k;
    const int bits[5] = {20, 18, 6, 10, 10};
    const float lb[5] = {-2500.f, -.3f, -5.f, 0.f, -32.f}, ub[5] = {2500.f, 1.3f, 5.f, 2.f, 32.f};
    for (int i = 0; i < 5; ++i) { c.bit_depths[i] = bits[i]; c.lower_bounds[i] = lb[i]; c.upper_bounds[i] = ub[i]; }
    return c;
}

static bool names(const char* word) { return std::strstr(smoe_last_error(), word) != nullptr; }

// every refusal of the entry point, with a real handle
static void drive(int dim, int ch, int b0, int b1, int b2, int precision) {
    smoe_config c = config(dim, ch, 4, b0, b1, b2);
    c.precision = precision;
    smoe_handle h = nullptr;
    EXPECT(smoe_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[4096];
    uint32_t act[64];
    uint8_t arg[64];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    smoe_params bad = p; bad.gamma_e = nullptr;
    const int32_t grid[3] = {3, 4, 2}, grid_zero[3] = {3, 0, 2}, grid_huge[3] = {65536, 65536, 2};
    const int32_t first[3] = {1, 0, 0}, first_neg[3] = {1, -1, 0}, first_far[3] = {1, 2, 0};
    const int32_t blocks[3] = {2, 3, 2}, blocks_zero[3] = {2, 0, 2};
    const int32_t s0[3] = {0, 5, 40}, s1[4] = {0, 7, 7, 300}, s2[3] = {0, 1, 3};       // an empty run, a run of 293 samples
    const int32_t s1_start[4] = {1, 7, 7, 300}, s1_dec[4] = {0, 7, 6, 300}, s1_none[4] = {0, 0, 0, 0};
    const int32_t* st[3] = {s0, s1, s2};
    const int32_t* st_null[3] = {s0, nullptr, s2};
    const int32_t* st_start[3] = {s0, s1_start, s2};
    const int32_t* st_dec[3] = {s0, s1_dec, s2};
    const int32_t* st_none[3] = {s0, s1_none, s2};
    const float* tabs[3] = {dummy, dummy, dummy};
    const float* tabs_null[3] = {dummy, nullptr, dummy};
    const float half[3] = {0.5f * b0, 0.5f * b1, 0.5f * b2};
    const float ok[3] = {1.5f, 2.0f, (b2 > 1) ? 1.0f : 0.0f}, zero[3] = {0.0f, 0.0f, 0.0f};
    auto call = [&](const smoe_params* pp, const int32_t* gg, const int32_t* ff, const int32_t* bb, const int32_t* const* ss,
                    const float* const* t, const float* bl, void* image, int fmt) {
        return smoe_render_view(h, pp, act, gg, ff, bb, ss, t, bl, image, fmt, arg, nullptr);
    };
    // what a correct call does up to the launch
    EXPECT(call(&p, grid, first, blocks, st, tabs, nullptr, dummy, SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(call(&p, grid, first, blocks, st, tabs, ok, dummy, SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(call(&p, grid, first, blocks, st, tabs, half, dummy, (precision <= 8) ? SMOE_IMAGE_U8 : SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(call(&p, grid, first, blocks, st, tabs, zero, dummy, SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(smoe_render_view(h, &p, nullptr, grid, first, blocks, st, tabs, ok, dummy, SMOE_IMAGE_F32, nullptr, nullptr) == SMOE_OK);
    // blend
    for (int l = 0; l < dim; ++l) {
        float b[3] = {ok[0], ok[1], ok[2]};
        const std::string word = "blend[" + std::to_string(l) + "]";
        b[l] = -0.25f;
        EXPECT(call(&p, grid, first, blocks, st, tabs, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(call(&p, grid, first, blocks, st, tabs, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::numeric_limits<float>::infinity();
        EXPECT(call(&p, grid, first, blocks, st, tabs, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::nextafter(half[l], 1e9f);
        EXPECT(call(&p, grid, first, blocks, st, tabs, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
    }
    if (dim == 2) {                                            // entries [dim .. 2] are ignored
        const float junk[3] = {1.0f, 1.0f, -7.0f};
        EXPECT(call(&p, grid, first, blocks, st, tabs, junk, dummy, 0) == SMOE_OK);
    }
    // nulls
    EXPECT(smoe_render_view(nullptr, &p, act, grid, first, blocks, st, tabs, ok, dummy, 0, arg, nullptr) == SMOE_ERR_INVALID && names("handle"));
    EXPECT(call(nullptr, grid, first, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(&bad, grid, first, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(&p, grid, first, blocks, st, tabs, ok, nullptr, 0) == SMOE_ERR_INVALID && names("image"));
    EXPECT(call(&p, nullptr, first, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("grid"));
    EXPECT(call(&p, grid, nullptr, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("view_first"));
    EXPECT(call(&p, grid, first, nullptr, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("view_blocks"));
    EXPECT(call(&p, grid, first, blocks, nullptr, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_start"));
    EXPECT(call(&p, grid, first, blocks, st, nullptr, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_coords"));
    EXPECT(call(&p, grid, first, blocks, st_null, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_start[1]"));
    EXPECT(call(&p, grid, first, blocks, st, tabs_null, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_coords[1]"));
    // values
    EXPECT(call(&p, grid_zero, first, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("grid[1]"));
    EXPECT(call(&p, grid_huge, first, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("2^31"));
    EXPECT(call(&p, grid, first_neg, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("view_first[1]"));
    EXPECT(call(&p, grid, first, blocks_zero, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("view_blocks[1]"));
    EXPECT(call(&p, grid, first_far, blocks, st, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("exceeds grid[1]"));
    EXPECT(call(&p, grid, first, blocks, st_start, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_start[1][0]"));
    EXPECT(call(&p, grid, first, blocks, st_dec, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_start[1] must not decrease"));
    EXPECT(call(&p, grid, first, blocks, st_none, tabs, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_start[1] must end"));
    EXPECT(call(&p, grid, first, blocks, st, tabs, ok, dummy, 7) == SMOE_ERR_INVALID && names("image_format"));
    if (precision > 8)
        EXPECT(call(&p, grid, first, blocks, st, tabs, ok, dummy, SMOE_IMAGE_U8) == SMOE_ERR_UNSUPPORTED && names("precision"));
    EXPECT(smoe_destroy(h) == SMOE_OK);
}

// the plan of a view, checked entry by entry
static void plan(int D, int C, int K, const std::vector<std::vector<int32_t>>& starts, const int32_t* first, const int32_t* grid,
                 const float* band, int hl) {
    int nv = 0;
    const smoe::Variant* vv = smoe::variants(&nv);
    const smoe::Variant* v = nullptr;
    for (int i = 0; i < nv && !v; ++i)
        if (vv[i].D == D && vv[i].C == C && vv[i].K == K) v = &vv[i];
    EXPECT(v != nullptr && v->render_view_layout != nullptr);
    if (!v) return;
    smoe::RenderViewArgs a;
    std::memset(&a, 0, sizeof a);
    smoe::ViewHost hst;
    std::memset(&hst, 0, sizeof hst);
    for (int l = 0; l < 3; ++l) { a.r.grid[l] = 1; a.r.ext[l] = 1; }
    for (int l = 0; l < D; ++l) {
        a.r.grid[l] = grid[l];
        a.r.ext[l] = starts[l].back();
        a.band[l] = band[l];
        hst.start[l] = starts[l].data(); hst.first[l] = first[l]; hst.blocks[l] = (int32_t)starts[l].size() - 1;
    }
    smoe::ViewPlan pl;
    smoe::RenderLayout g;
    std::memset(&g, 0, sizeof g);
    const hipError_t e = v->render_view_layout(a, hst, pl, hl, g);
    EXPECT(e == hipSuccess);
    if (e != hipSuccess) return;
    EXPECT(g.lds_bytes <= 160u * 1024u && g.workgroups >= 1);
    EXPECT(a.r.CL >= 1 && a.r.RP >= 1 && a.r.CL * a.r.RP <= 256);
    EXPECT(a.r.off_par % 4 == 0 && a.r.off_stage >= a.r.off_par);
    const std::vector<int32_t>& t = pl.tab;
    long long wgs = 1;
    size_t nrec_max = 1;
    for (int l = 0; l < D; ++l) {
        const int E = starts[l].back();
        const int nt = a.ntiles[l];
        wgs *= nt;
        const int32_t* ts = &t[a.o_tile_s[l]];
        const int32_t* te = &t[a.o_tile_e[l]];
        const int32_t* es = &t[a.o_ent_start[l]];
        const int32_t* sl = &t[a.o_ent_slot[l]];
        const int32_t* rb = &t[a.o_rec_block[l]];
        EXPECT(ts[0] == 0 && ts[nt] == E);
        int nr_max = 0;
        bool ok = true;
        for (int i = 0; i < nt; ++i) {
            const int e0 = te[2 * i], e1 = te[2 * i + 1];
            ok = ok && ts[i] < ts[i + 1] && ts[i + 1] - ts[i] <= a.TS[l] && e0 < e1;
            ok = ok && es[e0] <= ts[i] && ts[i + 1] <= es[e1];            // every sample of the tile lies in one of its entries
            for (int en = e0; en < e1 && ok; ++en) ok = es[en] < es[en + 1];                 // entries are non-empty runs
            const bool halo = band[l] > 0.0f;
            const int b0 = rb[sl[e0]], b1 = rb[sl[e1 - 1]];
            const int r0 = sl[e0] - ((halo && b0 > 0) ? 1 : 0), r1 = sl[e1 - 1] + ((halo && b1 < grid[l] - 1) ? 1 : 0);
            ok = ok && r0 >= 0 && (!halo || b0 == 0 || rb[r0] == b0 - 1) && (!halo || b1 == grid[l] - 1 || rb[r1] == b1 + 1);
            for (int r = r0; r < r1 && ok; ++r) ok = rb[r] < rb[r + 1] && rb[r + 1] < grid[l];
            nr_max = std::max(nr_max, r1 - r0 + 1);
            if (l == D - 1) ok = ok && ts[i + 1] - ts[i] <= a.r.CL;
        }
        EXPECT(ok);
        if (l + 1 < D) EXPECT(a.off_ax[l] + 3 * a.TS[l] + nr_max <= a.off_ax[l + 1]);
        else EXPECT(a.off_ax[l] + 3 * a.TS[l] + nr_max <= a.r.off_par);
        nrec_max *= (size_t)nr_max;
        // the entries are the non-empty runs of the caller's table, in order
        int en = 0;
        for (size_t j = 0; j + 1 < starts[l].size(); ++j)
            if (starts[l][j + 1] > starts[l][j]) { EXPECT(es[en] == starts[l][j] && rb[sl[en]] == first[l] + (int)j); ++en; }
        EXPECT(es[en] == E);
    }
    EXPECT(wgs == g.workgroups);
    EXPECT((size_t)(a.r.off_stage - a.r.off_par) * sizeof(float) <= 48u * 1024u && (size_t)(a.r.off_stage - a.r.off_par) % nrec_max == 0);
    EXPECT(g.lds_bytes >= sizeof(float) * (size_t)a.r.off_stage);
}

static std::vector<int32_t> uniform(int blocks, int run) {
    std::vector<int32_t> s(blocks + 1);
    for (int j = 0; j <= blocks; ++j) s[j] = j * run;
    return s;
}

int main() {
    drive(2, 1, 16, 16, 1, 8);
    drive(2, 3, 7, 5, 1, 8);
    drive(3, 3, 16, 16, 4, 8);
    drive(3, 1, 12, 10, 1, 10);                                // one frame per block: no blending on that axis
    const float none[3] = {0, 0, 0}, all[3] = {0.1f, 0.1f, 0.1f}, rows[3] = {0.1f, 0, 0};
    const int32_t z[3] = {0, 0, 0};
    for (const float* band : {none, all, rows}) {
        // empty runs (a thumbnail: 20 samples over 135 blocks), a 1-sample axis
        {
            std::vector<int32_t> thumb(136, 0);
            for (int j = 1; j <= 135; ++j) thumb[j] = (j * 20) / 135;
            const int32_t grid[3] = {135, 240, 1};
            plan(2, 3, 4, {thumb, uniform(240, 1)}, z, grid, band, 1);
            plan(2, 3, 4, {{0, 1}, uniform(240, 8)}, z, grid, band, 0);
            const int32_t first[3] = {134, 239, 0};
            plan(2, 1, 4, {{0, 1}, {0, 1}}, first, grid, band, 1);
        }
        // one block owns a run of more than 512 samples; 64x into one block
        {
            const int32_t grid[3] = {3, 4, 1}, first[3] = {1, 1, 0};
            plan(2, 1, 4, {{0, 3, 6, 9}, {0, 52, 574, 600}}, z, grid, band, 1);
            plan(2, 3, 4, {{0, 1024}, {0, 1024}}, first, grid, band, 1);
        }
        // the cfg4-sized view at 1x and 8x, video
        {
            const int32_t grid[3] = {135, 240, 1};
            plan(2, 3, 4, {uniform(68, 16), uniform(120, 16)}, z, grid, band, 1);
            plan(2, 3, 4, {uniform(9, 128), uniform(15, 128)}, z, grid, band, 1);
            const int32_t g3[3] = {4, 5, 6};
            plan(3, 3, 4, {uniform(4, 9), uniform(5, 33), uniform(6, 1)}, z, g3, band, 2);
            plan(3, 3, 4, {uniform(4, 9), {0, 0, 0, 7, 7, 8}, uniform(6, 300)}, z, g3, band, 1);
        }
        // the largest records (3-d, six kernels, three channels), every axis blended, many blocks per tile: the largest LDS case
        {
            const int32_t g3[3] = {40, 40, 40};
            plan(3, 3, 6, {uniform(40, 2), uniform(40, 3), uniform(40, 7)}, z, g3, band, 2);
            plan(3, 1, 8, {uniform(40, 1), uniform(40, 1), uniform(40, 1)}, z, g3, band, 0);
        }
    }
    EXPECT(smoe_abi_version() == 2);
    std::printf("viewcheck: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
