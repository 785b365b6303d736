// shared_sample_area_each_args_driver.cpp -- the argument checks and the host plan of smoe_shared_sample_area_each
// (csrc/smoe_capi.hip, csrc/smoe_shared_sample_area_each.hip.h) on a box WITHOUT a GPU, under AddressSanitizer +
// UndefinedBehaviorSanitizer: linked with the host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1: handles without a
// device, launches compiled out), so every call runs up to the point where it would launch.  footprints and taps are DEVICE
// arrays: the host layer must never read them, so they are handed in as one-element static arrays (a NaN, a 255): a read past
// them lands in ASan's redzone, a read of them would show as an argument error.  The
// plan itself (smoe::shared_sample_area_each_layout) is also run directly: the LDS need and the workgroup count.  Built by
// `make -C steered_mixture_of_experts_amd/csrc hostcheck_shared_sample_area_each`.  Test infrastructure:
// tests/test_shared_sample_area_each_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "smoe_device.h"
#include "smoe_hip.h"

// The constants of the default build.  plan() checks the workgroup count and the LDS bytes of every call against them exactly,
// so a library built with other -DSMOE_SSE_POINTS / -DSMOE_SSE_PPL2 / -DSMOE_SSE_PPL3 fails here instead of testing other edges.
static const int POINTS = 64;                  // SSE_POINTS: points per workgroup
static int tile(int D) { return D == 2 ? 256 : 512; }      // SSE_TILE: work items (taps) per round, one / two per lane

static int g_checks = 0, g_fail = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, smoe_last_error()); } \
    } while (0)

static smoe_shared_config config(int dim, int ch, int k, const int* image, const int* batch, int precision) {
    smoe_shared_config c;
    std::memset(&c, 0, sizeof c);
    c.abi_version = SMOE_ABI_VERSION;
    c.dim = dim;
    for (int l = 0; l < 3; ++l) { c.image_shape[l] = (l < dim) ? image[l] : 1; c.batch_shape[l] = (l < dim) ? batch[l] : 1; }
    c.channels = ch; c.kernels = k; c.precision = precision; c.margin = 0.5f;
    c.use_determinant = 1; c.train_pis = c.train_gammas = c.train_musx = 1;
    c.lr_expert = 1e-3f; c.lr_pis = 1e-5f; c.lr_steer = 1.0f; c.beta1 = 0.9f; c.beta2 = 0.999f; c.adam_eps = 1e-8f;
    c.start_pis = k;
    const int bits[5] = {20, 18, 6, 10, 10};
    const float lb[5] = {-2500.f, -.3f, -5.f, 0.f, -32.f}, ub[5] = {2500.f, 1.3f, 5.f, 2.f, 32.f};
    for (int i = 0; i < 5; ++i) { c.bit_depths[i] = bits[i]; c.lower_bounds[i] = lb[i]; c.upper_bounds[i] = ub[i]; }
    return c;
}

static bool names(const char* word) { return std::strstr(smoe_last_error(), word) != nullptr; }

// every refusal of the entry point, with a real handle; a correct call after each refused one
static void drive(int dim, int ch, int k, const int* image, const int* batch, int precision) {
    smoe_shared_config c = config(dim, ch, k, image, batch, precision);
    smoe_shared_handle h = nullptr;
    EXPECT(smoe_shared_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[4096], val[4096], mean[4096];
    static uint32_t lists[4096];
    static uint8_t cnt[4096];
    static int32_t ids[4096];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    smoe_params bad = p; bad.nu_e = nullptr;
    // the device arrays: one element each, so that a host read past it (or of NaN / 255 taken as an argument error) shows
    static const float foot[1] = {__builtin_nanf("")};
    static const uint8_t taps[1] = {255};
    // misaligned addresses are fine: "any 4-byte address" / "any address"
    const float* foot1 = dummy + 1;
    const uint8_t* taps3 = cnt + 3;

    auto call = [&](smoe_shared_handle hh, const smoe_params* pp, const float* points, int64_t n, const float* f,
                    const uint8_t* t, void* v, int32_t fmt, float* m) {
        return smoe_shared_sample_area_each(hh, pp, lists, points, n, f, t, v, fmt, m, cnt, ids, nullptr);
    };
    auto ok = [&]() { return call(h, &p, dummy, 64, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_OK; };
    EXPECT(ok());                                                               // what a correct call does up to the launch
    for (int64_t n : {(int64_t)1, (int64_t)POINTS - 1, (int64_t)POINTS, (int64_t)POINTS + 1, (int64_t)3077})
        EXPECT(call(h, &p, dummy, n, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    EXPECT(call(h, &p, dummy, 64, foot1, taps3, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    EXPECT(call(h, &p, dummy, 64, foot, taps, nullptr, SMOE_IMAGE_F32, mean) == SMOE_OK);     // the mean alone
    EXPECT(call(h, &p, dummy, 64, foot, taps, val, SMOE_IMAGE_F32, nullptr) == SMOE_OK);      // the values alone
    EXPECT(smoe_shared_sample_area_each(h, &p, nullptr, dummy, 64, foot, taps, val, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(call(h, &p, nullptr, 0, nullptr, nullptr, nullptr, SMOE_IMAGE_F32, nullptr) == SMOE_OK);   // no points: needs no array
    EXPECT((call(h, &p, dummy, 64, foot, taps, val, SMOE_IMAGE_U8, mean) == SMOE_OK) == (precision <= 8));
    if (precision > 8) {
        EXPECT(names("precision") && names("smoe_shared_sample_area_each"));
        EXPECT(call(h, &p, dummy, 64, foot, taps, nullptr, SMOE_IMAGE_U8, mean) == SMOE_OK);  // no values: the format is not used
    }
    EXPECT(call(nullptr, &p, dummy, 64, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("handle")
           && names("smoe_shared_sample_area_each"));
    EXPECT(ok());
    EXPECT(call(h, nullptr, dummy, 64, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(h, &bad, dummy, 64, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("p "));
    EXPECT(ok());
    EXPECT(call(h, &p, nullptr, 64, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("points"));
    EXPECT(call(h, &p, dummy, 64, nullptr, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("footprints"));
    EXPECT(call(h, &p, dummy, 64, foot, nullptr, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("taps"));
    EXPECT(ok());
    EXPECT(call(h, &p, dummy, 64, foot, taps, nullptr, SMOE_IMAGE_F32, nullptr) == SMOE_ERR_INVALID && names("values or mean"));
    EXPECT(call(h, &p, dummy, 64, foot, taps, val, 7, mean) == SMOE_ERR_INVALID && names("image_format"));
    EXPECT(call(h, &p, dummy, 0, nullptr, nullptr, val, 7, mean) == SMOE_ERR_INVALID && names("image_format"));   // also without points
    EXPECT(call(h, &p, dummy, -1, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("num_points"));
    EXPECT(ok());
    // 2^31 workgroups
    EXPECT(call(h, &p, dummy, (int64_t)0x7fffffff * POINTS, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    EXPECT(call(h, &p, dummy, (int64_t)0x7fffffff * POINTS + 1, foot, taps, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_UNSUPPORTED
           && names("2^31") && names("smoe_shared_sample_area_each"));
    EXPECT(ok());
    EXPECT(smoe_shared_destroy(h) == SMOE_OK);
}

// an axis of more than 2^24 pixels: the point form refuses (batch origins are not exact in fp32)
static void wide() {
    const int image[3] = {16, (1 << 24) + 16, 1}, batch[3] = {16, 16, 1};
    smoe_shared_config c = config(2, 1, 1, image, batch, 8);
    smoe_shared_handle h = nullptr;
    EXPECT(smoe_shared_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[64], val[64];
    static uint8_t tp[64];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    EXPECT(smoe_shared_sample_area_each(h, &p, nullptr, dummy, 8, dummy, tp, val, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr)
           == SMOE_ERR_UNSUPPORTED && names("2^24"));
    EXPECT(smoe_shared_sample_area_each(h, &p, nullptr, nullptr, 0, nullptr, nullptr, nullptr, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(smoe_shared_destroy(h) == SMOE_OK);
}

// the carve-up the header states: list | records | counters | offset table | footprints, centres, tap counts | prefix | staging
static size_t plan_floats(int D, int C, int K) {
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    const size_t taps = (size_t)tile(D) * (size_t)(C + 1) + POINTS, outs = (size_t)POINTS * (size_t)(2 * C + 2);
    return (size_t)K + 64u * SP + 8u + 256u + (size_t)POINTS * (size_t)(D * D + D + 1) + (size_t)(POINTS + 4) + (taps > outs ? taps : outs);
}

// the plan of a call
static void plan(int D, int C, int K, long long N, bool fits) {
    smoe::RenderLayout g;
    std::memset(&g, 0, sizeof g);
    const hipError_t e = smoe::shared_sample_area_each_layout(D, C, K, N, g);
    const size_t floats = plan_floats(D, C, K);
    EXPECT(g.workgroups == (N + POINTS - 1) / POINTS && g.hl == 0);
    EXPECT(g.lds_bytes >= sizeof(float) * floats && g.lds_bytes < sizeof(float) * (floats + 4) && g.lds_bytes % 16 == 0);
    EXPECT((e == hipSuccess) == fits);
    EXPECT(fits || e == hipErrorNotSupported);
}

int main() {
    const int i2[3] = {64, 96, 1}, b2[3] = {16, 16, 1}, i2r[3] = {21, 25, 1}, b2r[3] = {7, 5, 1};
    const int i3[3] = {32, 48, 8}, b3[3] = {16, 16, 4};
    drive(2, 1, 48, i2, b2, 8);
    drive(2, 3, 9, i2r, b2r, 8);
    drive(3, 3, 32, i3, b3, 8);
    drive(3, 1, 144, i3, b3, 10);
    wide();
    for (int D = 2; D <= 3; ++D)
        for (int C = 1; C <= 3; C += 2) {
            for (long long N : {0LL, 1LL, (long long)POINTS - 1, (long long)POINTS, (long long)POINTS + 1, 3077LL, 2160LL * 3840})
                plan(D, C, 144, N, true);
            plan(D, C, 8192, 0x7fffffffLL * POINTS, true);               // 2^31 - 1 workgroups, the largest kernel set a handle takes
            plan(D, C, 8192, 0x7fffffffLL * POINTS + 1, false);          // 2^31 workgroups
            const int Kedge = (int)(40960u - plan_floats(D, C, 0));      // 160 KB exactly
            plan(D, C, Kedge, 4096, true);
            plan(D, C, Kedge + 1, 4096, false);
            plan(D, C, 40000, 4096, false);
        }
    EXPECT(smoe_abi_version() == 2);
    std::printf("sharedsampleareaeachcheck: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
