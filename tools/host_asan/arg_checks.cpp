// Stand-alone host program for a sanitizer build of the library's HOST code (tools/host_asan/run.sh: -fsanitize=address,undefined on the
// host side only): drives the argument checks and the host-side index arithmetic of f3dg_forward_sets / f3dg_backward_sets /
// f3dg_render_epilogue_backward / f3dg_workspace_bytes. Every call below returns before the first HIP call, so it needs no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "f3dg.h"

static int failures = 0;
#define EXPECT(call, want)                                                                     \
    do {                                                                                       \
        const long long got_ = (long long)(call);                                              \
        if (got_ != (long long)(want)) { printf("FAIL %s: got %lld, want %lld\n", #call, got_, (long long)(want)); failures++; } \
    } while (0)

static int forward_sets(void* ws, size_t ws_bytes, int n_sets, int vps, int P, const float* v2g, unsigned flags, long long cap = 1000)
{
    float* p = static_cast<float*>(ws);
    return f3dg_forward_sets(nullptr, ws, ws_bytes, cap, n_sets, vps, P, 1, 4, p, 64, 64, p, p, nullptr, p, p, 1.0f, p, nullptr, v2g, p, p, p,
                             0.1f, 0.1f, 0.0f, p, nullptr, flags);
}

struct Outs { float *mean2D, *opacity, *color, *mean3D, *sh, *scale, *rot, *v2g; };

static int backward_sets(void* ws, size_t ws_bytes, int n_sets, int vps, int P, const float* v2g_precomp, Outs o, const float* dpix,
                         const float* means3D, long long cap = 1000, int W = 64, int H = 64)
{
    float* p = static_cast<float*>(ws);
    return f3dg_backward_sets(nullptr, ws, ws_bytes, cap, n_sets, vps, P, 1, 4, p, W, H, means3D, p, nullptr, p, 1.0f, p, nullptr, v2g_precomp,
                              p, p, p, 0.1f, 0.1f, 0.0f, nullptr, dpix, o.mean2D, nullptr, o.opacity, o.color, o.mean3D, nullptr, o.sh,
                              o.scale, o.rot, o.v2g, 0u);
}

int main()
{
    std::vector<float> buf(256, 0.0f);
    void* ws = buf.data();
    float* p = buf.data();
    const unsigned AUX = F3DG_FLAG_SAVE_AUX, SETS = F3DG_FLAG_SETS_AUX;
    const size_t huge = (size_t)1 << 40;

    // ---- f3dg_forward_sets: the flag rules
    EXPECT(forward_sets(ws, huge, 1, 1, 100, nullptr, SETS), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, huge, 2, 1, 100, nullptr, SETS), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, huge, 2, 1, 100, nullptr, AUX), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, huge, 2, 1, 100, p, AUX | SETS), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, huge, 2, 1, 100, p, 0u), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, 1024, 2, 1, 100, nullptr, AUX | SETS), F3DG_ERR_WORKSPACE);
    EXPECT(forward_sets(ws, 1024, 1, 2, 100, nullptr, AUX | SETS), F3DG_ERR_WORKSPACE);
    EXPECT(forward_sets(ws, huge, 0, 1, 100, nullptr, 0u), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, huge, 1, 0, 100, nullptr, 0u), F3DG_ERR_BAD_ARG);
    EXPECT(forward_sets(ws, huge, 65536, 65536, 100, nullptr, 0u), F3DG_ERR_BAD_ARG);          // n_sets * views_per_set beyond int
    EXPECT(forward_sets(ws, 1024, 40000, 40000, 3, nullptr, AUX | SETS), F3DG_ERR_BAD_ARG);    // (view, Gaussian) index beyond 32 bits
    EXPECT(forward_sets(ws, 1024, 8, 4, 65536, nullptr, AUX | SETS, 4000000), F3DG_ERR_WORKSPACE);      // the layout arithmetic at a real size

    // ---- f3dg_backward_sets
    const Outs all = { p, p, p, p, p, p, p, p };
    EXPECT(backward_sets(ws, 1024, 2, 2, 100, nullptr, all, p, p), F3DG_ERR_WORKSPACE);
    EXPECT(backward_sets(ws, 1024, 1, 4, 100, nullptr, all, p, p), F3DG_ERR_WORKSPACE);
    EXPECT(backward_sets(ws, 1024, 1, 4, 100, p, all, p, p), F3DG_ERR_WORKSPACE);              // one set may have view2gaussian_precomp
    EXPECT(backward_sets(ws, 1024, 2, 2, 100, p, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 0, 2, 100, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 2, 0, 100, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 2, -1, 100, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 65536, 65536, 100, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 70000, 1, 100, nullptr, all, p, p), F3DG_ERR_BAD_ARG);     // the set is a grid's y coordinate
    EXPECT(backward_sets(ws, 1024, 40000, 40000, 3, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 2, 2, -1, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 2, 2, 0, nullptr, all, p, p), F3DG_OK);                     // no Gaussians: nothing to do
    EXPECT(backward_sets(ws, 1024, 2, 2, 100, nullptr, all, nullptr, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 2, 2, 100, nullptr, all, p, nullptr), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(nullptr, 1024, 2, 2, 100, nullptr, all, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(backward_sets(ws, 1024, 2, 2, 100, nullptr, all, p, p, 1000, 0, 64), F3DG_ERR_BAD_ARG);
    for (int k = 0; k < 8; k++) {
        Outs o = all;
        (&o.mean2D)[k] = nullptr;
        EXPECT(backward_sets(ws, 1024, 2, 2, 100, nullptr, o, p, p), F3DG_ERR_BAD_ARG);
    }
    EXPECT(backward_sets(ws, 1024, 8, 4, 65536, nullptr, all, p, p, 4000000, 256, 256), F3DG_ERR_WORKSPACE);
    // f3dg_backward is the one-set case of the same code
    EXPECT(f3dg_backward(nullptr, ws, 1024, 1000, 3, 100, 1, 4, p, 64, 64, p, p, nullptr, p, 1.0f, p, nullptr, nullptr, p, p, p, 0.1f, 0.1f, 0.0f,
                         nullptr, p, p, nullptr, p, p, p, nullptr, p, p, p, p, 0u), F3DG_ERR_WORKSPACE);
    EXPECT(f3dg_backward(nullptr, ws, 1024, 1000, 0, 100, 1, 4, p, 64, 64, p, p, nullptr, p, 1.0f, p, nullptr, nullptr, p, p, p, 0.1f, 0.1f, 0.0f,
                         nullptr, p, p, nullptr, p, p, p, nullptr, p, p, p, p, 0u), F3DG_ERR_BAD_ARG);

    // ---- f3dg_render_epilogue_backward
    EXPECT(f3dg_render_epilogue_backward(nullptr, 0, 8, 8, p, p, 1.0f, 1.0f, p, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(f3dg_render_epilogue_backward(nullptr, 1, 8, 8, nullptr, p, 1.0f, 1.0f, p, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(f3dg_render_epilogue_backward(nullptr, 1, 8, 8, p, nullptr, 1.0f, 1.0f, p, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(f3dg_render_epilogue_backward(nullptr, 1, 8, 8, p, p, 1.0f, 1.0f, p, p, nullptr), F3DG_ERR_BAD_ARG);
    EXPECT(f3dg_render_epilogue_backward(nullptr, 1, 65536, 65536, p, p, 1.0f, 1.0f, p, p, p), F3DG_ERR_BAD_ARG);
    EXPECT(f3dg_render_epilogue_backward(nullptr, 1, 8, 8, p, p, 1.0f, 1.0f, nullptr, nullptr, p), F3DG_OK);       // nothing to add

    // ---- the workspace of the bench shape: 8 sets x 4 views
    EXPECT(f3dg_workspace_bytes(65536, 256, 256, 32, 4000000) > f3dg_workspace_bytes(65536, 256, 256, 4, 4000000), 1);

    if (failures) printf("%d FAILURES\n", failures);
    else printf("host argument checks: all passed\n");
    return failures ? 1 : 0;
}
