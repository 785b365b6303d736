// sample_area_each_args_driver.cpp -- the argument checks and the host plan of smoe_sample_area_each (csrc/smoe_capi.hip,
// csrc/smoe_sample_area_each.hip.h) on a box WITHOUT a GPU, under AddressSanitizer + UndefinedBehaviorSanitizer: linked with
// the host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1: handles without a device, launches compiled out), so every
// call runs up to the point where it would launch.  The plan itself (Variant::sample_area_each_layout) is also run directly:
// the record budget, the LDS carve-up with the offset table, the footprint slots and the tap counts behind the staging, and
// the workgroup count.  Built by `make -C steered_mixture_of_experts_amd/csrc hostcheck_sample_area_each`.  Test
// infrastructure: tests/test_sample_area_each_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

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

static bool names(const char* word) {
    return std::strstr(smoe_last_error(), word) != nullptr && std::strstr(smoe_last_error(), "smoe_sample_area_each") != nullptr;
}

// every refusal of the entry point, with a real handle.  points, footprints, taps and the outputs are device arrays: the host
// layer never reads them, whatever they hold (the void rule is the kernel's)
static void drive(int dim, int ch, int b0, int b1, int b2, int precision) {
    smoe_config c = config(dim, ch, 4, b0, b1, b2);
    c.precision = precision;
    smoe_handle h = nullptr;
    EXPECT(smoe_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[4096];
    static uint8_t cnt[4096], tp[4096];
    uint32_t act[64];
    int32_t blk[64];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    smoe_params bad = p; bad.nu_e = nullptr;
    const int bs[3] = {b0, b1, b2};
    const int32_t grid[3] = {3, 4, 2}, grid_zero[3] = {3, 0, 2}, grid_huge[3] = {65536, 65536, 2};
    const int32_t len[3] = {3 * b0 - (b0 > 1 ? 1 : 0), 4 * b1, 2 * b2}, len_zero[3] = {len[0], 0, len[2]};
    const int32_t len_big[3] = {len[0], 4 * b1 + 1, len[2]};
    const int32_t grid_wide[3] = {3, (1 << 24) / b1 + 1, 2}, len_wide[3] = {len[0], 64, len[2]};    // grid * n > 2^24 on axis 1
    const int32_t grid_edge[3] = {3, (1 << 24) / b1, 2};                                            // grid * n <= 2^24: accepted
    const float half[3] = {0.5f * b0, 0.5f * b1, 0.5f * b2};
    const float ok[3] = {1.5f, 2.0f, (b2 > 1) ? 1.0f : 0.0f};
    float* F = dummy;
    auto call = [&](const smoe_params* pp, const int32_t* gg, const int32_t* ll, const float* pts, int64_t n, const float* fp,
                    const uint8_t* tt, const float* bl, void* values, int32_t fmt = SMOE_IMAGE_F32) {
        return smoe_sample_area_each(h, pp, act, gg, ll, pts, n, fp, tt, bl, values, fmt, dummy, cnt, blk, nullptr);
    };
    // what a correct call does up to the launch
    EXPECT(call(&p, grid, len, dummy, 64, F, tp, nullptr, dummy) == SMOE_OK);
    EXPECT(call(&p, grid, len, dummy, 64, F, tp, ok, dummy) == SMOE_OK);
    EXPECT(call(&p, grid, len, dummy, 1, F, tp, half, dummy) == SMOE_OK);
    EXPECT(call(&p, grid, len, dummy, 3 * 1024 + 5, F, tp, nullptr, dummy) == SMOE_OK);
    EXPECT(call(&p, grid_edge, len_wide, dummy, 64, F, tp, ok, dummy) == SMOE_OK);
    if (precision <= 8) EXPECT(call(&p, grid, len, dummy, 64, F, tp, ok, dummy, SMOE_IMAGE_U8) == SMOE_OK);
    // footprints at any 4-byte address, taps at any address
    for (int sh = 0; sh < 5; ++sh) EXPECT(call(&p, grid, len, dummy, 64, F + sh, tp + sh, ok, dummy) == SMOE_OK);
    // mean, count and block are optional, and so is values beside mean
    EXPECT(smoe_sample_area_each(h, &p, nullptr, grid, len, dummy, 64, F, tp, ok, dummy, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(smoe_sample_area_each(h, &p, nullptr, grid, len, dummy, 64, F, tp, ok, nullptr, SMOE_IMAGE_F32, dummy, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(smoe_sample_area_each(h, &p, nullptr, grid, len, dummy, 64, F, tp, ok, nullptr, SMOE_IMAGE_U8, dummy, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(smoe_sample_area_each(h, &p, act, grid, len, dummy, 64, F, tp, ok, nullptr, SMOE_IMAGE_F32, nullptr, cnt, blk, nullptr) == SMOE_ERR_INVALID
           && names("values") && names("mean"));
    // no points: a no-op that needs neither points, footprints, taps nor outputs
    EXPECT(smoe_sample_area_each(h, &p, act, grid, len, nullptr, 0, nullptr, nullptr, ok, nullptr, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    // the test hook
    for (const char* v : {"0", "1", "7", "100000", "-3", "junk", ""}) {
        setenv("SMOE_SAMPLE_RECORDS", v, 1);
        EXPECT(call(&p, grid, len, dummy, 64, F, tp, ok, dummy) == SMOE_OK);
    }
    unsetenv("SMOE_SAMPLE_RECORDS");
    // footprints and taps
    EXPECT(call(&p, grid, len, dummy, 64, nullptr, tp, ok, dummy) == SMOE_ERR_INVALID && names("footprints"));
    EXPECT(call(&p, grid, len, dummy, 64, F, nullptr, ok, dummy) == SMOE_ERR_INVALID && names("taps"));
    EXPECT(call(&p, grid, len, dummy, 1, nullptr, nullptr, ok, dummy) == SMOE_ERR_INVALID && names("footprints"));
    // blend
    for (int l = 0; l < dim; ++l) {
        float b[3] = {ok[0], ok[1], ok[2]};
        const std::string word = "blend[" + std::to_string(l) + "]";
        b[l] = -0.25f;
        EXPECT(call(&p, grid, len, dummy, 64, F, tp, b, dummy) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(call(&p, grid, len, dummy, 64, F, tp, b, dummy) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::nextafter(half[l], 1e9f);
        EXPECT(call(&p, grid, len, dummy, 64, F, tp, b, dummy) == SMOE_ERR_INVALID && names(word.c_str()));
    }
    // nulls
    EXPECT(smoe_sample_area_each(nullptr, &p, act, grid, len, dummy, 64, F, tp, ok, dummy, SMOE_IMAGE_F32, dummy, cnt, blk, nullptr) == SMOE_ERR_INVALID && names("handle"));
    EXPECT(call(nullptr, grid, len, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(&bad, grid, len, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(&p, nullptr, len, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("grid"));
    EXPECT(call(&p, grid, nullptr, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("length"));
    EXPECT(call(&p, grid, len, nullptr, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("points"));
    // values
    EXPECT(call(&p, grid_zero, len, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("grid[1]"));
    EXPECT(call(&p, grid_huge, len, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("2^31"));
    EXPECT(call(&p, grid, len_zero, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("length[1]"));
    EXPECT(call(&p, grid, len_big, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("length[1]"));
    EXPECT(call(&p, grid, len, dummy, -1, F, tp, ok, dummy) == SMOE_ERR_INVALID && names("num_points"));
    EXPECT(call(&p, grid, len, dummy, 64, F, tp, ok, dummy, 7) == SMOE_ERR_INVALID && names("image_format"));
    // not supported
    if (bs[1] > 1) EXPECT(call(&p, grid_wide, len_wide, dummy, 64, F, tp, ok, dummy) == SMOE_ERR_UNSUPPORTED && names("2^24"));
    if (precision > 8) EXPECT(call(&p, grid, len, dummy, 64, F, tp, ok, dummy, SMOE_IMAGE_U8) == SMOE_ERR_UNSUPPORTED && names("precision"));
    EXPECT(call(&p, grid, len, dummy, (int64_t)1 << 39, F, tp, ok, dummy) == SMOE_ERR_UNSUPPORTED && names("2^31"));
    EXPECT(call(&p, grid, len, dummy, ((int64_t)1 << 39) - 256, F, tp, ok, dummy) == SMOE_OK);          // 2^31 - 1 workgroups
    EXPECT(smoe_destroy(h) == SMOE_OK);
}

// the plan of a call
static void plan(int D, int C, int K, const int32_t* grid, const float* band, long long N, long long records, long long want_cap) {
    int nv = 0;
    const smoe::Variant* vv = smoe::variants(&nv);
    const smoe::Variant* v = nullptr;
    for (int i = 0; i < nv && !v; ++i)
        if (vv[i].D == D && vv[i].C == C && vv[i].K == K) v = &vv[i];
    EXPECT(v != nullptr && v->sample_area_each_layout != nullptr && v->sample_area_each != nullptr);
    if (!v) return;
    smoe::SampleAreaEachArgs a;
    std::memset(&a, 0, sizeof a);
    for (int l = 0; l < 3; ++l) { a.s.r.grid[l] = 1; a.s.n[l] = 1; }
    long long total = 1;
    for (int l = 0; l < D; ++l) { a.s.r.grid[l] = grid[l]; a.s.band[l] = band[l]; total *= grid[l]; }
    a.s.num_points = N;
    smoe::RenderLayout g;
    std::memset(&g, 0, sizeof g);
    const hipError_t e = v->sample_area_each_layout(a, records, g);
    EXPECT(e == hipSuccess);
    if (e != hipSuccess) return;
    EXPECT(g.workgroups == (N + 255) / 256 && g.hl == 0);
    EXPECT(a.s.r.off_par >= 2 * D && a.s.r.off_par % 4 == 0 && a.s.r.off_stage >= a.s.r.off_par && a.s.r.off_stage % 4 == 0);
    const size_t rec_bytes = sizeof(float) * (size_t)(a.s.r.off_stage - a.s.r.off_par);
    EXPECT(rec_bytes <= 12u * 1024u && a.s.rec_cap >= 0 && a.s.rec_cap <= total);
    EXPECT(a.s.rec_cap == 0 || rec_bytes % (size_t)a.s.rec_cap == 0);
    EXPECT(records < 0 || a.s.rec_cap <= records);
    EXPECT(want_cap < 0 || a.s.rec_cap == want_cap);
    // the staging (values, mean, count, block of 256 points), the offset table [16][16], a footprint slot of D * D floats per lane,
    // the tap counts of 256 points as bytes: none overlaps the next, the last ends with the dynamic LDS
    EXPECT(a.off_tab % 4 == 0 && a.off_tab >= a.s.r.off_stage + 256 * (2 * C + 2) && a.off_tab < a.s.r.off_stage + 256 * (2 * C + 2) + 4);
    EXPECT(a.off_fp == a.off_tab + 16 * 16 && a.off_tap == a.off_fp + 256 * D * D);
    EXPECT(g.lds_bytes == sizeof(float) * (size_t)a.off_tap + (size_t)(256 * D) && g.lds_bytes % 4 == 0 && g.lds_bytes <= 160u * 1024u);
}

int main() {
    drive(2, 1, 16, 16, 1, 8);
    drive(2, 3, 7, 5, 1, 8);
    drive(3, 3, 16, 16, 4, 8);
    drive(3, 1, 12, 10, 1, 10);                                // one frame per block; precision 10: no U8 values
    const float none[3] = {0, 0, 0}, all[3] = {0.1f, 0.1f, 0.1f};
    const int32_t small[3] = {3, 4, 1}, big[3] = {135, 240, 1}, g3[3] = {40, 40, 40}, line[3] = {1, 2, 1};
    for (const float* band : {none, all})
        for (const char* hook : {"", "5", "0"}) {              // SMOE_SAMPLE_RECORDS reaches the plan as `records`
            const long long rec = hook[0] ? std::atoll(hook) : -1;
            plan(2, 3, 4, small, band, 1, rec, rec < 0 ? 12 : rec);        // never more records than blocks
            plan(2, 3, 4, small, band, 3 * 1024 + 5, 4, 4);
            plan(2, 3, 4, small, band, 5063, 0, 0);
            plan(2, 3, 4, big, band, 270LL * 480, rec, rec < 0 ? -1 : rec);
            plan(2, 3, 4, big, band, 270LL * 480, 1, 1);
            plan(2, 1, 4, line, band, 100, -1, 2);
            plan(3, 3, 6, g3, band, 1 << 20, rec, -1);         // the largest records
            plan(3, 3, 8, g3, band, 1 << 20, rec, -1);         // the largest staging and footprint slots beside them
            plan(3, 1, 8, g3, band, 1 << 20, rec, -1);
            plan(3, 3, 4, g3, band, (1LL << 39) - 256, rec, -1);
        }
    EXPECT(smoe_abi_version() == 2);
    std::printf("sampleareaeachcheck: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
