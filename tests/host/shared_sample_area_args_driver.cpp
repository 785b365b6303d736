// shared_sample_area_args_driver.cpp -- the argument checks and the host plan of smoe_shared_sample_area (csrc/smoe_capi.hip,
// csrc/smoe_shared_sample_area.hip.h) on a box WITHOUT a GPU, under AddressSanitizer + UndefinedBehaviorSanitizer: linked with
// the host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1: handles without a device, launches compiled out), so every
// call runs up to the point where it would launch.  The plan itself (smoe::shared_sample_area_layout) is also run directly: the
// LDS need and the workgroup count for T = 1, 9 and 64 taps.  Built by
// `make -C steered_mixture_of_experts_amd/csrc hostcheck_shared_sample_area`.  Test infrastructure:
// tests/test_shared_sample_area_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "smoe_device.h"
#include "smoe_hip.h"

static const int TILE = 512;                   // SSA_TILE: work items (taps) per workgroup

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
    const float F[9] = {3.f, -1.f, 0.f, 1.f, 3.f, 0.5f, 0.f, 0.25f, 1.5f};
    const int32_t tp[3] = {3, 2, 2}, one[3] = {1, 1, 1};
    int32_t full[3] = {8, 8, 1};
    if (dim == 3) { full[0] = 4; full[1] = 4; full[2] = 4; }

    auto call = [&](smoe_shared_handle hh, const smoe_params* pp, const float* points, int64_t n, const float* f,
                    const int32_t* t, void* v, int32_t fmt, float* m) {
        return smoe_shared_sample_area(hh, pp, lists, points, n, f, t, v, fmt, m, cnt, ids, nullptr);
    };
    auto ok = [&]() { return call(h, &p, dummy, 64, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_OK; };
    EXPECT(ok());                                                               // what a correct call does up to the launch
    EXPECT(call(h, &p, dummy, 1, F, one, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    EXPECT(call(h, &p, dummy, 3 * 512 + 5, F, full, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    EXPECT(call(h, &p, dummy, 64, F, tp, nullptr, SMOE_IMAGE_F32, mean) == SMOE_OK);          // the mean alone
    EXPECT(call(h, &p, dummy, 64, F, tp, val, SMOE_IMAGE_F32, nullptr) == SMOE_OK);           // the values alone
    EXPECT(smoe_shared_sample_area(h, &p, nullptr, dummy, 64, F, tp, val, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(call(h, &p, nullptr, 0, F, tp, nullptr, SMOE_IMAGE_F32, nullptr) == SMOE_OK);      // no points: needs no plane
    EXPECT((call(h, &p, dummy, 64, F, tp, val, SMOE_IMAGE_U8, mean) == SMOE_OK) == (precision <= 8));
    if (precision > 8) {
        EXPECT(names("precision") && names("smoe_shared_sample_area"));
        EXPECT(call(h, &p, dummy, 64, F, tp, nullptr, SMOE_IMAGE_U8, mean) == SMOE_OK);       // no values: the format is not used
    }
    EXPECT(call(nullptr, &p, dummy, 64, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("handle")
           && names("smoe_shared_sample_area"));
    EXPECT(ok());
    EXPECT(call(h, nullptr, dummy, 64, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(h, &bad, dummy, 64, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("p "));
    EXPECT(ok());
    EXPECT(call(h, &p, nullptr, 64, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("points"));
    EXPECT(call(h, &p, dummy, 64, nullptr, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("footprint"));
    EXPECT(call(h, &p, dummy, 64, F, nullptr, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("taps"));
    EXPECT(call(h, &p, dummy, 0, nullptr, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("footprint"));   // also without points
    EXPECT(ok());
    EXPECT(call(h, &p, dummy, 64, F, tp, nullptr, SMOE_IMAGE_F32, nullptr) == SMOE_ERR_INVALID && names("values or mean"));
    EXPECT(call(h, &p, dummy, 64, F, tp, val, 7, mean) == SMOE_ERR_INVALID && names("image_format"));
    EXPECT(call(h, &p, dummy, -1, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("num_points"));
    EXPECT(ok());
    for (int m = 0; m < dim; ++m) {
        const std::string w = "taps[" + std::to_string(m) + "]";
        for (int v : {0, -2, 17}) {
            int32_t t[3] = {2, 2, 2};
            t[m] = v;
            EXPECT(call(h, &p, dummy, 64, F, t, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names(w.c_str()));
        }
    }
    {
        const int32_t many2[3] = {9, 8, 1}, many3[3] = {4, 4, 5}, edge2[3] = {16, 4, 1}, edge3[3] = {16, 2, 2};
        EXPECT(call(h, &p, dummy, 64, F, dim == 2 ? many2 : many3, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names("64"));
        EXPECT(call(h, &p, dummy, 64, F, dim == 2 ? edge2 : edge3, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    }
    for (int e = 0; e < dim * dim; ++e)
        for (float v : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
            float f[9];
            std::memcpy(f, F, sizeof f);
            f[e] = v;
            const std::string w = "footprint[" + std::to_string(e / dim) + "][" + std::to_string(e % dim) + "]";
            EXPECT(call(h, &p, dummy, 64, f, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_INVALID && names(w.c_str()));
        }
    EXPECT(ok());
    // 2^31 workgroups: T = 12 (d = 3) / 6 (d = 2) taps -> 42 / 85 points per workgroup
    const int T = (dim == 3) ? 12 : 6, P = TILE / T;
    EXPECT(call(h, &p, dummy, (int64_t)0x7fffffff * P, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_OK);
    EXPECT(call(h, &p, dummy, (int64_t)0x7fffffff * P + 1, F, tp, val, SMOE_IMAGE_F32, mean) == SMOE_ERR_UNSUPPORTED && names("2^31"));
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
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    const float F[4] = {2.f, 0.f, 0.f, 2.f};
    const int32_t tp[2] = {2, 2};
    EXPECT(smoe_shared_sample_area(h, &p, nullptr, dummy, 8, F, tp, val, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr)
           == SMOE_ERR_UNSUPPORTED && names("2^24"));
    EXPECT(smoe_shared_sample_area(h, &p, nullptr, nullptr, 0, F, tp, nullptr, SMOE_IMAGE_F32, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(smoe_shared_destroy(h) == SMOE_OK);
}

static size_t plan_floats(int D, int C, int K, int T) {
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C, P = TILE / T;
    const size_t taps = (size_t)P * (size_t)(T * (C + 1) + 1), outs = (size_t)P * (size_t)(2 * C + 2);
    return (size_t)K + 64u * SP + 8u + (size_t)(D * D * 16) + (taps > outs ? taps : outs);
}

// the plan of a call
static void plan(int D, int C, int K, int T, long long N, bool fits) {
    smoe::RenderLayout g;
    std::memset(&g, 0, sizeof g);
    const hipError_t e = smoe::shared_sample_area_layout(D, C, K, T, N, g);
    const int P = TILE / T;
    const size_t floats = plan_floats(D, C, K, T);
    EXPECT(g.workgroups == (N + P - 1) / P && g.hl == 0);
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
    smoe::RenderLayout g;
    EXPECT(smoe::shared_sample_area_layout(2, 1, 8, 0, 10, g) == hipErrorInvalidValue);
    EXPECT(smoe::shared_sample_area_layout(2, 1, 8, 65, 10, g) == hipErrorInvalidValue);
    for (int D = 2; D <= 3; ++D)
        for (int C = 1; C <= 3; C += 2)
            for (int T : {1, 9, 64}) {
                const long long P = TILE / T;
                for (long long N : {0LL, 1LL, P - 1, P, P + 1, 3077LL, 2160LL * 3840}) plan(D, C, 144, T, N, true);
                plan(D, C, 8192, T, 0x7fffffffLL * P, true);            // 2^31 - 1 workgroups, the largest kernel set a handle takes
                plan(D, C, 8192, T, 0x7fffffffLL * P + 1, false);       // 2^31 workgroups
                const int Kedge = (int)(40960u - plan_floats(D, C, 0, T));     // 160 KB exactly
                plan(D, C, Kedge, T, 4096, true);
                plan(D, C, Kedge + 1, T, 4096, false);
                plan(D, C, 40000, T, 4096, false);
            }
    EXPECT(smoe_abi_version() == 2);
    std::printf("sharedsampleareacheck: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
