// blend_args_driver.cpp -- the argument checks of smoe_render_blend (csrc/smoe_capi.hip) on a box WITHOUT a GPU, under
// AddressSanitizer + UndefinedBehaviorSanitizer: linked with the host-only objects of `make hostcheck` (-DSMOE_HOST_TEST=1:
// handles without a device, launches compiled out), so every call runs up to the point where it would launch.  Built by
// `make -C steered_mixture_of_experts_amd/csrc hostcheck_blend`.  Test infrastructure: tests/test_blend_render_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

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

static void drive(int dim, int ch, int b0, int b1, int b2, int precision) {
    smoe_config c = config(dim, ch, 4, b0, b1, b2);
    c.precision = precision;
    smoe_handle h = nullptr;
    EXPECT(smoe_create(&h, &c) == SMOE_OK && h != nullptr);
    if (!h) return;
    static float dummy[4096];                                  // covers every pointer the entry forms for 24 blocks of this size
    uint32_t act[64];
    uint8_t arg[64];
    smoe_params p = {dummy, dummy, dummy, dummy, dummy, dummy};
    smoe_params bad = p; bad.gamma_e = nullptr;
    const float* tabs[3] = {dummy, dummy, dummy};
    const float* tabs_null[3] = {dummy, nullptr, dummy};
    const int32_t m[3] = {24, 20, 7}, m_zero[3] = {24, 0, 7};
    const int32_t grid[3] = {3, 4, 2}, grid_zero[3] = {3, 0, 2}, grid_huge[3] = {65536, 65536, 2};
    const int total = (dim == 3) ? 24 : 12;
    const int64_t ext[3] = {3 * 24 - 5, 4 * 20 - 1, 2 * 7}, ext_big[3] = {3 * 24 + 1, 4 * 20, 2 * 7}, ext_zero[3] = {0, 80, 14};
    const int64_t ext_huge[3] = {65536LL * 24, 65536LL * 20, 14};
    const float half[3] = {0.5f * b0, 0.5f * b1, 0.5f * b2};
    const float ok[3] = {1.5f, 2.0f, (b2 > 1) ? 1.0f : 0.0f}, zero[3] = {0.0f, 0.0f, 0.0f};
    auto call = [&](int first, int count, const smoe_params* pp, const float* const* t, const int32_t* mm, const int32_t* gg,
                    const int64_t* ee, const float* bl, void* image, int fmt) {
        return smoe_render_blend(h, first, count, pp, act, t, mm, gg, ee, bl, image, fmt, arg, nullptr);
    };
    // what a correct call does up to the launch
    EXPECT(call(0, total, &p, tabs, m, grid, ext, ok, dummy, SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(call(3, total - 5, &p, tabs, m, grid, ext, half, dummy, (precision <= 8) ? SMOE_IMAGE_U8 : SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(call(2, 5, &p, tabs, m, grid, ext, zero, dummy, SMOE_IMAGE_F32) == SMOE_OK);            // all zero: smoe_render's path
    EXPECT(call(0, 0, &p, tabs, m, grid, ext, ok, dummy, SMOE_IMAGE_F32) == SMOE_OK);
    EXPECT(smoe_render_blend(h, 0, total, &p, nullptr, tabs, m, grid, ext, ok, dummy, SMOE_IMAGE_F32, nullptr, nullptr) == SMOE_OK);
    // blend
    EXPECT(call(0, total, &p, tabs, m, grid, ext, nullptr, dummy, 0) == SMOE_ERR_INVALID && names("blend"));
    for (int l = 0; l < dim; ++l) {
        float b[3] = {ok[0], ok[1], ok[2]};
        const std::string word = "blend[" + std::to_string(l) + "]";
        b[l] = -0.25f;
        EXPECT(call(0, total, &p, tabs, m, grid, ext, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(call(0, total, &p, tabs, m, grid, ext, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::numeric_limits<float>::infinity();
        EXPECT(call(0, total, &p, tabs, m, grid, ext, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
        b[l] = std::nextafter(half[l], 1e9f);
        EXPECT(call(0, total, &p, tabs, m, grid, ext, b, dummy, 0) == SMOE_ERR_INVALID && names(word.c_str()));
    }
    if (dim == 2) {                                            // entries [dim .. 2] are ignored
        const float junk[3] = {1.0f, 1.0f, -7.0f};
        EXPECT(call(0, total, &p, tabs, m, grid, ext, junk, dummy, 0) == SMOE_OK);
    }
    // every check of smoe_render
    EXPECT(smoe_render_blend(nullptr, 0, 1, &p, act, tabs, m, grid, ext, ok, dummy, 0, arg, nullptr) == SMOE_ERR_INVALID && names("handle"));
    EXPECT(call(-1, 1, &p, tabs, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("first_block"));
    EXPECT(call(0, -1, &p, tabs, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("num_blocks"));
    EXPECT(call(0, total, nullptr, tabs, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(0, total, &bad, tabs, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("p "));
    EXPECT(call(0, total, &p, tabs, m, grid, ext, ok, nullptr, 0) == SMOE_ERR_INVALID && names("image"));
    EXPECT(call(0, total, &p, nullptr, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_coords"));
    EXPECT(call(0, total, &p, tabs, nullptr, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("samples"));
    EXPECT(call(0, total, &p, tabs, m, nullptr, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("grid"));
    EXPECT(call(0, total, &p, tabs, m, grid, nullptr, ok, dummy, 0) == SMOE_ERR_INVALID && names("extent"));
    EXPECT(call(0, total, &p, tabs, m, grid, ext, ok, dummy, 7) == SMOE_ERR_INVALID && names("image_format"));
    EXPECT(call(0, total, &p, tabs_null, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("axis_coords[1]"));
    EXPECT(call(0, total, &p, tabs, m_zero, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("samples[1]"));
    EXPECT(call(0, total, &p, tabs, m, grid_zero, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("grid[1]"));
    EXPECT(call(0, total, &p, tabs, m, grid, ext_big, ok, dummy, 0) == SMOE_ERR_INVALID && names("extent[0]"));
    EXPECT(call(0, total, &p, tabs, m, grid, ext_zero, ok, dummy, 0) == SMOE_ERR_INVALID && names("extent[0]"));
    EXPECT(call(0, 1, &p, tabs, m, grid_huge, ext_huge, ok, dummy, 0) == SMOE_ERR_INVALID && names("2^31"));
    EXPECT(call(1, total, &p, tabs, m, grid, ext, ok, dummy, 0) == SMOE_ERR_INVALID && names("first_block + num_blocks"));
    if (precision > 8)
        EXPECT(call(0, total, &p, tabs, m, grid, ext, ok, dummy, SMOE_IMAGE_U8) == SMOE_ERR_UNSUPPORTED && names("precision"));
    EXPECT(smoe_destroy(h) == SMOE_OK);
}

int main() {
    drive(2, 1, 16, 16, 1, 8);
    drive(2, 3, 7, 5, 1, 8);
    drive(3, 3, 16, 16, 4, 8);
    drive(3, 1, 12, 10, 1, 10);                                // one frame per block: no blending on that axis, whatever blend[2] <= 1/2
    EXPECT(smoe_abi_version() == 2);
    std::printf("blendcheck: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
