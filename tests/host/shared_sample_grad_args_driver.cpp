// shared_sample_grad_args_driver.cpp -- the argument checks and the host plan of smoe_shared_sample_grad /
// smoe_shared_render_view_grad (csrc/smoe_capi.hip, csrc/smoe_shared_sample_grad.hip.h) on a box WITHOUT a GPU, under
// AddressSanitizer + UndefinedBehaviorSanitizer: linked with the host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1:
// handles without a device, launches compiled out), so every call runs up to the point where it would launch.  The plan itself
// (smoe::shared_sample_grad_layout) is also run directly: the LDS need and the workgroup count.  Built by
// `make -C steered_mixture_of_experts_amd/csrc hostcheck_shared_sample_grad`.  Test infrastructure:
// tests/test_shared_sample_grad_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "smoe_device.h"
#include "smoe_hip.h"

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

// every refusal of the two entry points, with a real handle; a correct call after each refused one
static void drive(int dim, int ch, int k, const int* image, const int* batch, int precision) {
    smoe_shared_config c = config(dim, ch, k, image, batch, precision);
    smoe_shared_handle h = nullptr;
    EXPECT(smoe_shared_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[4096], jac[4096];
    static uint32_t lists[4096];
    static int32_t ids[4096], tab[64];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    smoe_params bad = p; bad.nu_e = nullptr;

    // ---- smoe_shared_sample_grad ----
    auto pts = [&](smoe_shared_handle hh, const smoe_params* pp, const float* points, int64_t n, float* j) {
        return smoe_shared_sample_grad(hh, pp, lists, points, n, j, dummy, ids, nullptr);
    };
    auto ok = [&]() { return pts(h, &p, dummy, 64, jac) == SMOE_OK; };
    EXPECT(ok());                                                               // what a correct call does up to the launch
    EXPECT(pts(h, &p, dummy, 1, jac) == SMOE_OK);
    EXPECT(pts(h, &p, dummy, 3 * 512 + 5, jac) == SMOE_OK);
    EXPECT(smoe_shared_sample_grad(h, &p, nullptr, dummy, 64, jac, nullptr, nullptr, nullptr) == SMOE_OK);   // no lists, values, ids
    EXPECT(pts(h, &p, nullptr, 0, nullptr) == SMOE_OK);                         // no points: needs neither points nor jac
    EXPECT(pts(nullptr, &p, dummy, 64, jac) == SMOE_ERR_INVALID && names("handle") && names("smoe_shared_sample_grad"));
    EXPECT(ok());
    EXPECT(pts(h, nullptr, dummy, 64, jac) == SMOE_ERR_INVALID && names("p "));
    EXPECT(pts(h, &bad, dummy, 64, jac) == SMOE_ERR_INVALID && names("p "));
    EXPECT(ok());
    EXPECT(pts(h, &p, nullptr, 64, jac) == SMOE_ERR_INVALID && names("points"));
    EXPECT(pts(h, &p, dummy, 64, nullptr) == SMOE_ERR_INVALID && names("jac"));
    EXPECT(ok());
    EXPECT(pts(h, &p, dummy, -1, jac) == SMOE_ERR_INVALID && names("num_points"));
    EXPECT(pts(h, &p, dummy, (int64_t)1 << 40, jac) == SMOE_ERR_UNSUPPORTED && names("2^31"));
    EXPECT(pts(h, &p, dummy, ((int64_t)1 << 40) - 512, jac) == SMOE_OK);        // 2^31 - 1 workgroups
    EXPECT(ok());

    // ---- smoe_shared_render_view_grad ----
    const int32_t ext[3] = {5, 7, 2}, ext_zero[3] = {5, 0, 2}, ext_neg[3] = {-3, 7, 2};
    const int32_t ext_huge[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, ext_edge[3] = {1 << 20, (1 << 20) - 1, 1};
    const float* const ax[3] = {dummy, dummy, dummy};
    const int32_t* const ab[3] = {tab, tab, tab};
    auto view = [&](smoe_shared_handle hh, const smoe_params* pp, const int32_t* e, const float* const* a,
                    const int32_t* const* b, float* j) {
        return smoe_shared_render_view_grad(hh, pp, lists, e, a, b, j, dummy, ids, nullptr);
    };
    auto vok = [&]() { return view(h, &p, ext, ax, ab, jac) == SMOE_OK; };
    EXPECT(vok());
    EXPECT(smoe_shared_render_view_grad(h, &p, nullptr, ext, ax, ab, jac, nullptr, nullptr, nullptr) == SMOE_OK);
    if (dim == 2) {                                            // entries [dim .. 2] are ignored
        const int32_t junk[3] = {5, 7, -9};
        const float* const ax2[3] = {dummy, dummy, nullptr};
        const int32_t* const ab2[3] = {tab, tab, nullptr};
        EXPECT(view(h, &p, junk, ax2, ab2, jac) == SMOE_OK);
        EXPECT(view(h, &p, ext_edge, ax, ab, jac) == SMOE_OK);                  // 2^31 - 2^11 workgroups
    }
    EXPECT(view(nullptr, &p, ext, ax, ab, jac) == SMOE_ERR_INVALID && names("handle") && names("smoe_shared_render_view_grad"));
    EXPECT(vok());
    EXPECT(view(h, nullptr, ext, ax, ab, jac) == SMOE_ERR_INVALID && names("p "));
    EXPECT(view(h, &bad, ext, ax, ab, jac) == SMOE_ERR_INVALID && names("p "));
    EXPECT(view(h, &p, nullptr, ax, ab, jac) == SMOE_ERR_INVALID && names("extent"));
    EXPECT(vok());
    EXPECT(view(h, &p, ext, nullptr, ab, jac) == SMOE_ERR_INVALID && names("axis_coords"));
    EXPECT(view(h, &p, ext, ax, nullptr, jac) == SMOE_ERR_INVALID && names("axis_batch"));
    EXPECT(view(h, &p, ext, ax, ab, nullptr) == SMOE_ERR_INVALID && names("jac"));
    EXPECT(vok());
    EXPECT(view(h, &p, ext_zero, ax, ab, jac) == SMOE_ERR_INVALID && names("extent[1]"));
    EXPECT(view(h, &p, ext_neg, ax, ab, jac) == SMOE_ERR_INVALID && names("extent[0]"));
    for (int l = 0; l < dim; ++l) {
        const float* a1[3] = {dummy, dummy, dummy};
        const int32_t* b1[3] = {tab, tab, tab};
        a1[l] = nullptr;
        const std::string wa = "axis_coords[" + std::to_string(l) + "]", wb = "axis_batch[" + std::to_string(l) + "]";
        EXPECT(view(h, &p, ext, a1, ab, jac) == SMOE_ERR_INVALID && names(wa.c_str()));
        b1[l] = nullptr;
        EXPECT(view(h, &p, ext, ax, b1, jac) == SMOE_ERR_INVALID && names(wb.c_str()));
        EXPECT(vok());
    }
    EXPECT(view(h, &p, ext_huge, ax, ab, jac) == SMOE_ERR_UNSUPPORTED && names("2^31"));
    EXPECT(vok());
    EXPECT(smoe_shared_destroy(h) == SMOE_OK);
}

// an axis of more than 2^24 pixels: the point form refuses (batch origins are not exact in fp32), the view does not
static void wide() {
    const int image[3] = {16, (1 << 24) + 16, 1}, batch[3] = {16, 16, 1};
    smoe_shared_config c = config(2, 1, 1, image, batch, 8);
    smoe_shared_handle h = nullptr;
    EXPECT(smoe_shared_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[64], jac[64];
    static int32_t tab[64];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    EXPECT(smoe_shared_sample_grad(h, &p, nullptr, dummy, 8, jac, nullptr, nullptr, nullptr) == SMOE_ERR_UNSUPPORTED && names("2^24"));
    EXPECT(smoe_shared_sample_grad(h, &p, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == SMOE_OK);
    const int32_t ext[3] = {4, 4, 1};
    const float* const ax[3] = {dummy, dummy, nullptr};
    const int32_t* const ab[3] = {tab, tab, nullptr};
    EXPECT(smoe_shared_render_view_grad(h, &p, nullptr, ext, ax, ab, jac, nullptr, nullptr, nullptr) == SMOE_OK);
    EXPECT(smoe_shared_destroy(h) == SMOE_OK);
}

// the plan of a call
static void plan(int D, int C, int K, long long N, bool fits) {
    smoe::RenderLayout g;
    std::memset(&g, 0, sizeof g);
    const hipError_t e = smoe::shared_sample_grad_layout(D, C, K, N, g);
    const int SP = D * (D + 1) / 2 + D + 1 + C + D * C;
    const size_t floats = (size_t)K + 64u * SP + 8u + 512u * (size_t)(D * C + C + 1);
    EXPECT(g.workgroups == (N + 511) / 512 && g.hl == 0);
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
            plan(D, C, 1, 1, true);
            plan(D, C, 144, 512, true);
            plan(D, C, 144, 513, true);
            plan(D, C, 8192, 2160LL * 3840, true);                  // the largest kernel set a handle takes
            plan(D, C, 8192, (1LL << 40) - 512, true);              // 2^31 - 1 workgroups
            plan(D, C, 8192, (1LL << 40) - 511, false);
            plan(D, C, 40000, 4096, false);                         // over 160 KB of LDS
        }
    EXPECT(smoe_abi_version() == 2);
    std::printf("sharedsamplegradcheck: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
