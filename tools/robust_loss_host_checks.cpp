// Stand-alone driver for the host-side argument checks of csrc/robust_loss.hip: every call is one the entry points refuse (or an empty
// one) before any launch, so it runs without a GPU.  Meant for a host sanitizer build:
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -O1 -g gfnet_amd/csrc/robust_loss.hip gfnet_amd/csrc/capi.hip \
//         tools/robust_loss_host_checks.cpp -o /tmp/robust_loss_host_checks && /tmp/robust_loss_host_checks
#include <cstdio>
#include <cstring>

#include "../include/gfnet_hip.h"

static int failures = 0;

static void expect(int got, int want, const char *what) {
    if (got != want) {
        std::printf("FAIL %s: returned %d, expected %d (%s)\n", what, got, want, gfn_last_error());
        ++failures;
    }
}

int main() {
    alignas(16) static float buf[64];
    const float *maps[8];
    float *grads[8];
    for (int k = 0; k < 8; ++k) maps[k] = buf, grads[k] = buf;
    const float *holed[8];
    std::memcpy(holed, maps, sizeof(maps));
    holed[1] = nullptr;
    const int64_t big = (int64_t)1 << 40;
    auto fwd = [&](const float *const *f, const float *const *c, int n, const float *H, const float *prev, int ph, int pw, float *stats, int B,
                   int h, int w, double eb, double cs, void *ws, int64_t nws) {
        return gfn_robust_loss_fwd(f, c, n, H, nullptr, prev, ph, pw, 0.1, buf, stats, B, h, w, 95.0, eb, 0.5, cs, 0.01, 0.85, 0.01, ws, nws, nullptr);
    };
    auto bwd = [&](const float *const *f, int n, const float *go, float *const *gf, int need, int B, int w, double cs) {
        return gfn_robust_loss_bwd(f, maps, n, buf, nullptr, nullptr, 0, 0, 0.1, buf, go, gf, grads, need, B, 4, w, 95.0, 95.0, 0.5, cs, 0.01, 0.85,
                                   nullptr);
    };
    expect(fwd(nullptr, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd null flows");
    expect(fwd(maps, nullptr, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd null certs");
    expect(fwd(holed, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd null flow 2");
    expect(fwd(holed, maps, 1, buf, nullptr, 0, 0, buf, 0, 4, 6, 95.0, 1e-3, buf, big), GFN_OK, "fwd hole past n_itr, B = 0");
    expect(fwd(maps, maps, 0, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd n_itr 0");
    expect(fwd(maps, maps, 9, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd n_itr 9");
    expect(fwd(maps, maps, 2, nullptr, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd null H");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, nullptr, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd null stats");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, -1, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd B < 0");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 2, 0, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd h = 0");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 1, 1, 32769, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd side > 32768");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 5, 16384, 16384, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd > 2^30 cells");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 0.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd target extent 0");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 0.0, buf, big), GFN_ERR_INVALID_ARG, "fwd cs = 0");
    expect(fwd(maps, maps, 2, buf, buf, 0, 4, buf, 2, 4, 6, 95.0, 1e-3, buf, big), GFN_ERR_INVALID_ARG, "fwd prev 0 x 4");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, nullptr, big), GFN_ERR_INVALID_ARG, "fwd null ws");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf + 1, big), GFN_ERR_INVALID_ARG, "fwd misaligned ws");
    expect(fwd(maps, maps, 2, buf, nullptr, 0, 0, buf, 2, 4, 6, 95.0, 1e-3, buf, 15), GFN_ERR_INVALID_ARG, "fwd short ws");
    expect(fwd(maps, maps, 8, buf, nullptr, 0, 0, buf, 0, 4, 6, 95.0, 1e-3, nullptr, 0), GFN_OK, "fwd B = 0");
    expect(bwd(maps, 2, nullptr, grads, 0x303, 2, 6, 1e-3), GFN_ERR_INVALID_ARG, "bwd null grad_out");
    expect(bwd(maps, 2, buf, grads, 0x4, 2, 6, 1e-3), GFN_ERR_INVALID_ARG, "bwd need past n_itr");
    expect(bwd(maps, 2, buf, grads, -1, 2, 6, 1e-3), GFN_ERR_INVALID_ARG, "bwd need < 0");
    expect(bwd(maps, 2, buf, nullptr, 0x303, 2, 6, 1e-3), GFN_ERR_INVALID_ARG, "bwd null gradient array");
    expect(bwd(maps, 8, buf, nullptr, 0xff00, 0, 6, 1e-3), GFN_OK, "bwd B = 0, certainties only");
    expect(bwd(maps, 2, buf, nullptr, 0, 2, 6, 1e-3), GFN_OK, "bwd need = 0");
    expect(bwd(holed, 2, buf, grads, 0x303, 2, 6, 1e-3), GFN_ERR_INVALID_ARG, "bwd null flow 2");
    expect(bwd(maps, 2, buf, grads, 0x303, 2, 0, 1e-3), GFN_ERR_INVALID_ARG, "bwd w = 0");
    expect(bwd(maps, 2, buf, grads, 0x303, 2, 6, -1.0), GFN_ERR_INVALID_ARG, "bwd cs < 0");
    expect(gfn_gt_warp_homography_fwd(nullptr, nullptr, buf, buf, nullptr, 2, 4, 6, 95.0, 95.0, 1, nullptr), GFN_ERR_INVALID_ARG, "warp null H");
    expect(gfn_gt_warp_homography_fwd(buf, nullptr, buf, nullptr, nullptr, 2, 4, 6, 95.0, 95.0, 1, nullptr), GFN_ERR_INVALID_ARG, "warp null prob");
    expect(gfn_gt_warp_homography_fwd(buf, nullptr, buf, buf, nullptr, 2, 4, -6, 95.0, 95.0, 1, nullptr), GFN_ERR_INVALID_ARG, "warp w < 0");
    expect(gfn_gt_warp_homography_fwd(buf, nullptr, buf, buf, nullptr, 0, 4, 6, 95.0, 95.0, 0, nullptr), GFN_OK, "warp B = 0");
    if (gfn_robust_loss_ws_bytes(2, 4, 6, 2) != 16 || gfn_robust_loss_ws_bytes(3, 37, 41, 8) != 18 * 16 || gfn_robust_loss_ws_bytes(0, 4, 6, 2) != 0) {
        std::printf("FAIL ws_bytes\n");
        ++failures;
    }
    std::printf("robust_loss host checks: %d failure(s)\n", failures);
    return failures != 0;
}
