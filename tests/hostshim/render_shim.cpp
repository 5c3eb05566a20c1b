// render_shim.cpp -- TEST INFRASTRUCTURE.  Compiles multigrid_amd/csrc/mgx_render.h (the per-pixel tile evaluation the atlas
// kernel runs) with g++ for tests/test_render_host.py: the host atlas is compared with the reference's recorded tiles.
#include <cstdint>

#include "../../multigrid_amd/csrc/mgx_render.h"

extern "C" {

// u8[RENDER_KEYS, ts, ts, 3]
int shim_render_atlas(int tile_size, uint8_t *out) {
    if (tile_size < 1 || tile_size > mgx::RENDER_MAX_TILE) return -1;
    const mgx::RenderTrig trig = mgx::render_trig_host();
    for (int k = 0; k < mgx::RENDER_KEYS; k++) mgx::render_tile(k, tile_size, trig, out + (int64_t)k * tile_size * tile_size * 3);
    return 0;
}

void shim_render_trig(double *c, double *s) {
    const mgx::RenderTrig t = mgx::render_trig_host();
    for (int d = 0; d < 4; d++) { c[d] = t.c[d]; s[d] = t.s[d]; }
}

int shim_render_appearance(int t, int c, int s) { return mgx::render_appearance((uint32_t)t, (uint32_t)c, (uint32_t)s); }

}
