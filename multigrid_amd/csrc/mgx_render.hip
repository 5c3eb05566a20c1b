// mgx_render.hip -- RGB frames of the envs (MultiGridEnv.get_full_render, multigrid/base.py:707-760), gfx950.
//
//   mgx_render_atlas   every tile the reference can draw (mgx_render.h: 2 500 keys) at one tile size, u8[2500, ts, ts, 3]: one lane
//                      per output pixel, the 3x3 supersampled pixels evaluated in float64 by the header the CPU tests build too.
//   mgx_render         u8[n, H*ts, W*ts, 3] from the grid, the agents and (for the highlight) the observation of the state: one
//                      workgroup per (env, cell row).  (1) The keys of the row's W cells, in LDS: the cell's appearance, the agent
//                      drawn on it (the highest-index live agent there, grid.py:281-283), and whether any agent -- terminated or
//                      not -- sees it (base.py:712-747: a view cell is visible where the observation's type is not `unseen`).
//                      (2) The row's band of the frame -- ts pixel rows of W*ts*3 bytes, contiguous -- copied from atlas rows:
//                      16-byte stores when ts % 4 == 0 (every dword then lies inside one tile row), byte stores otherwise.
//
// The frames are written once and never read back, so the 16-byte stores can be non-temporal; MGX_RENDER_STORES=plain selects
// plain ones (tools/render_bench.py compares the two).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mgx_aux_geom.h"
#include "mgx_host.h"
#include "mgx_render.h"
#include "mgx_rules.h"

namespace {

using namespace mgx;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void render_atlas_kernel(int ts, int total, RenderTrig trig, uint8_t *__restrict__ atlas) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int tt = ts * ts;
    const int key = i / tt, pix = i - key * tt;
    const int oy = pix / ts, ox = pix - oy * ts;
    const int hl = key & 1, ov = (key >> 1) % RENDER_OVERLAYS, ap = (key >> 1) / RENDER_OVERLAYS;
    const uint32_t c = render_pixel(ap, ov, hl, ox, oy, ts, trig);
    uint8_t *p = atlas + 3 * (int64_t)i;
    p[0] = (uint8_t)c;
    p[1] = (uint8_t)(c >> 8);
    p[2] = (uint8_t)(c >> 16);
}

// n / d with magic = recip32(d) (mgx_aux_geom.h): here n < W * d <= 255 * d and d = 3 * ts <= 192, inside recip32_exact_below(d)
__device__ __forceinline__ uint32_t div_small(uint32_t n, uint32_t magic) { return __umulhi(n, magic); }

// CB: bytes per cell (1 compact, 2 MgxCell, 3 byte triples); VEC: 16-byte stores (ts % 4 == 0, aligned); NT: non-temporal.
template <int CB, bool VEC, bool NT>
__global__ __launch_bounds__(256) void render_kernel(int W, int H, int A, int v, int ts, const uint8_t *__restrict__ grid,
                                                     const uint8_t *__restrict__ agents, const uint8_t *__restrict__ obs,
                                                     const uint8_t *__restrict__ atlas, uint8_t *__restrict__ frames,
                                                     uint32_t magic_T3, float inv_R) {
    __shared__ uint8_t s_agents[MGX_MAX_AGENTS * 8];
    __shared__ uint16_t s_keys[256];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x;                                      // (env, cell row)
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    if (t < A * 8) s_agents[t] = agents[b * A * 8 + t];
    __syncthreads();

    // (1) keys of the row's cells
    for (int x = t; x < W; x += 256) {
        const uint32_t cell = load_cell_shown(CB, grid + ((b * H + y) * W + x) * CB);
        const int ap = render_appearance(cell & 0xffu, (cell >> 8) & 0xffu, (cell >> 16) & 0xffu);
        int ov = 0;
        for (int a = A - 1; a >= 0; a--) {                               // last writer wins among the live agents on the cell
            const uint8_t *r = s_agents + 8 * a;
            if (r[AG_X] == x && r[AG_Y] == y && !r[AG_TERM]) {
                ov = r[AG_COLOR] <= 5 ? 1 + 4 * r[AG_COLOR] + (r[AG_DIR] & 3) : 0;
                break;
            }
        }
        int hl = 0;
        if (obs) {
            for (int a = 0; a < A && !hl; a++) {
                const uint8_t *r = s_agents + 8 * a;
                const int d = r[AG_DIR] & 3, fx = dir_dx(d), fy = dir_dy(d), rx = -fy, ry = fx;
                const int tlx = r[AG_X] + fx * (v - 1) - rx * (v / 2), tly = r[AG_Y] + fy * (v - 1) - ry * (v / 2);
                const int dx = x - tlx, dy = y - tly;
                const int vi = dx * rx + dy * ry, vj = -(dx * fx + dy * fy);  // abs = top_left - f * vj + r * vi
                if (vi >= 0 && vi < v && vj >= 0 && vj < v)
                    hl = obs[(((b * A + a) * v + vi) * v + vj) * 3] != (uint8_t)T_UNSEEN;
            }
        }
        s_keys[x] = (uint16_t)render_key(ap, ov, hl);
    }
    __syncthreads();

    // (2) the band: ts pixel rows of R bytes
    const int T3 = 3 * ts, R = W * T3;
    const int tile_bytes = ts * T3;
    uint8_t *band = frames + row * (int64_t)ts * R;
    if constexpr (VEC) {
        // the band is ts * R bytes, a multiple of 16 (ts % 4 == 0); a 16-byte chunk may cross tile and pixel-row boundaries, a dword
        // never does (R and 3 * ts are multiples of 4)
        const int total = ts * R / 16;
        for (int i = t; i < total; i += 256) {
            const int o = 16 * i;
            int py = __float2int_rz((float)o * inv_R);                    // o < 2^22: exact in float, the quotient off by <= 1
            if (py * R > o) py--;
            else if ((py + 1) * R <= o) py++;
            int tile = (int)div_small((uint32_t)(o - py * R), magic_T3);
            int off = o - py * R - tile * T3;
            u32x4 w;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (off >= T3) {
                    off -= T3;
                    if (++tile == W) { tile = 0; py++; }
                }
                w[k] = *reinterpret_cast<const uint32_t *>(atlas + (int)s_keys[tile] * tile_bytes + py * T3 + off);
                off += 4;
            }
            u32x4 *dst = reinterpret_cast<u32x4 *>(band + o);
            if constexpr (NT)
                __builtin_nontemporal_store(w, dst);
            else
                *dst = w;
        }
    } else {
        for (int py = 0; py < ts; py++) {
            for (int bx = t; bx < R; bx += 256) {
                const int tile = (int)div_small((uint32_t)bx, magic_T3);
                band[(int64_t)py * R + bx] = atlas[(int)s_keys[tile] * tile_bytes + py * T3 + (bx - tile * T3)];
            }
        }
    }
}

// the planar atlas, u8[2500, 3, ts, ts]: the same pixels as render_atlas_kernel's, one plane per channel (what mgx_render_views blits
// into channels-first frames)
__global__ __launch_bounds__(256) void render_atlas_planar_kernel(int ts, int total, RenderTrig trig, uint8_t *__restrict__ atlas) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int tt = ts * ts;
    const int key = i / tt, pix = i - key * tt;
    const int oy = pix / ts, ox = pix - oy * ts;
    const int hl = key & 1, ov = (key >> 1) % RENDER_OVERLAYS, ap = (key >> 1) / RENDER_OVERLAYS;
    const uint32_t c = render_pixel(ap, ov, hl, ox, oy, ts, trig);
    uint8_t *p = atlas + 3 * (int64_t)key * tt + pix;
    p[0] = (uint8_t)c;
    p[tt] = (uint8_t)(c >> 8);
    p[2 * tt] = (uint8_t)(c >> 16);
}

// ---------------------------------------------------------------------------------------------------------------- view frames
// mgx_render_views: every agent's view as the frame the viewer sees, u8[n_views, P, P, 3] or (planar) u8[n_views, 3, P, P], P = v * ts.
// A frame is a stack of ROWS of R = v * U bytes, each a run of v tile rows of U bytes: U = 3 * ts and P rows per frame in the
// interleaved layout, U = ts and 3 * P rows (channel-major) in the planar one, whose atlas is planar too -- one blit for both.
//
// Geometry: a workgroup of 256 lanes takes G WHOLE consecutive views (views_per_group: as many as make about 32 KiB of frame, 1..16),
// never a part of one: a 7 x 7 view at ts = 8 is 9 408 bytes = 588 16-byte chunks, 2.3 per lane -- alone it leaves a third of the last
// pass idle, and a view ROW (1 344 bytes) would not fill one pass.  The group's frames are contiguous, so its G * F bytes are one
// range cut into 16-byte chunks, a chunk per lane and pass; G * F < 2^22 (one view is at most 3 * 960 * 960 bytes; G > 1 only below
// 32 KiB), which keeps every offset exact in float and the quotients below one correction step.  (1) The keys of the G views' cells,
// at most 16 * 225, in LDS (render_view_key, mgx_render.h).  (2) The blit: 16-byte stores when ts % 4 == 0 -- F is then a multiple
// of 16 and every dword lies inside one tile row (U is a multiple of 4) -- and `frames` is 16-byte aligned, byte stores otherwise.
constexpr int kViewGroupBytes = 32768, kViewGroupMax = 16;

inline int views_per_group(int64_t frame_bytes) {
    const int64_t g = (kViewGroupBytes + frame_bytes - 1) / frame_bytes;
    return g < 1 ? 1 : (g > kViewGroupMax ? kViewGroupMax : (int)g);
}

struct ViewFrameGeom {
    int v, ts, planar;
    int U, R, NR, P, F, tile_bytes;      // tile-row bytes, frame-row bytes, rows per frame, pixels per side, frame bytes, atlas tile bytes
    float inv_U, inv_R, inv_P, inv_F, inv_ts;
};

// n / d for 0 <= n < 2^22 with inv = 1.0f / d: n is exact in float, the product is off by less than one
__device__ __forceinline__ int div_near(int n, int d, float inv) {
    int q = __float2int_rz((float)n * inv);
    if (q * d > n) q--;
    else if ((q + 1) * d <= n) q++;
    return q;
}

// frame row gy -> the tile row j of the view cells it crosses and the row `ar` of their atlas tiles (planar: channel * ts + tile row)
__device__ __forceinline__ void view_row(const ViewFrameGeom &g, int gy, int &j, int &ar) {
    int ch = 0, py = gy;
    if (g.planar) {
        ch = div_near(gy, g.P, g.inv_P);
        py = gy - ch * g.P;
    }
    j = div_near(py, g.ts, g.inv_ts);
    ar = ch * g.ts + (py - j * g.ts);
}

template <bool VEC, bool NT>
__global__ __launch_bounds__(256) void render_views_kernel(ViewFrameGeom g, int64_t n_views, int G, int highlight,
                                                           const uint8_t *__restrict__ obs, const uint8_t *__restrict__ dir,
                                                           const uint8_t *__restrict__ color, int64_t color_period,
                                                           const uint8_t *__restrict__ atlas, uint8_t *__restrict__ frames) {
    __shared__ uint16_t s_keys[kViewGroupMax * MGX_MAX_VIEW * MGX_MAX_VIEW];
    __shared__ uint8_t s_dir[kViewGroupMax], s_col[kViewGroupMax];
    const int t = threadIdx.x;
    const int64_t view0 = (int64_t)blockIdx.x * G;
    const int Gn = n_views - view0 < G ? (int)(n_views - view0) : G;      // (the last group may be short)
    if (t < Gn) {
        s_dir[t] = dir[view0 + t];
        s_col[t] = color[(view0 + t) % color_period];
    }
    __syncthreads();

    // (1) keys: image[i, j] of view k at s_keys[k * v * v + i * v + j]
    const int VV = g.v * g.v, own = (g.v / 2) * g.v + g.v - 1;
    for (int c = t; c < Gn * VV; c += 256) {
        const int k = c / VV, cell = c - k * VV;
        const uint8_t *p = obs + ((view0 + k) * VV + cell) * 3;
        s_keys[c] = (uint16_t)render_view_key(p[0], p[1], p[2], cell == own, s_dir[k], s_col[k], highlight != 0);
    }
    __syncthreads();

    // (2) the blit of the group's Gn * F bytes
    uint8_t *out = frames + view0 * (int64_t)g.F;
    const int total = Gn * g.F;
    if constexpr (VEC) {
        for (int ci = t; ci < total / 16; ci += 256) {
            const int o = 16 * ci;
            int k = G > 1 ? div_near(o, g.F, g.inv_F) : 0;
            const int r = o - k * g.F;
            int gy = div_near(r, g.R, g.inv_R);
            const int xb = r - gy * g.R;
            int i = div_near(xb, g.U, g.inv_U);
            int off = xb - i * g.U;
            int j, ar;
            view_row(g, gy, j, ar);
            u32x4 w;
#pragma unroll
            for (int d = 0; d < 4; d++) {
                if (off >= g.U) {                                        // the next tile; the next row; the next view
                    off = 0;
                    if (++i == g.v) {
                        i = 0;
                        if (++gy == g.NR) { gy = 0; k++; }
                        view_row(g, gy, j, ar);
                    }
                }
                w[d] = *reinterpret_cast<const uint32_t *>(atlas + (int)s_keys[k * VV + i * g.v + j] * g.tile_bytes + ar * g.U + off);
                off += 4;
            }
            u32x4 *dst = reinterpret_cast<u32x4 *>(out + o);
            if constexpr (NT)
                __builtin_nontemporal_store(w, dst);
            else
                *dst = w;
        }
    } else {
        for (int o = t; o < total; o += 256) {
            const int k = G > 1 ? div_near(o, g.F, g.inv_F) : 0;
            const int r = o - k * g.F;
            const int gy = div_near(r, g.R, g.inv_R);
            const int xb = r - gy * g.R;
            const int i = div_near(xb, g.U, g.inv_U);
            int j, ar;
            view_row(g, gy, j, ar);
            out[o] = atlas[(int)s_keys[k * VV + i * g.v + j] * g.tile_bytes + ar * g.U + (xb - i * g.U)];
        }
    }
}

template <int CB>
using RenderKernel = void (*)(int, int, int, int, int, const uint8_t *, const uint8_t *, const uint8_t *, const uint8_t *, uint8_t *,
                              uint32_t, float);

template <int CB>
RenderKernel<CB> pick(bool vec, bool nt) {
    return vec ? (nt ? render_kernel<CB, true, true> : render_kernel<CB, true, false>) : render_kernel<CB, false, false>;
}

}  // namespace

extern "C" {

int mgx_render_atlas(int32_t tile_size, uint8_t *atlas, void *stream) {
    if (tile_size < 1 || tile_size > RENDER_MAX_TILE || !atlas) return MGX_ERR_INVALID_ARGUMENT;
    const int total = RENDER_KEYS * tile_size * tile_size;
    hipLaunchKernelGGL(render_atlas_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       tile_size, total, render_trig_host(), atlas);
    return finish_launch();
}

int mgx_render(const MgxSpec *spec, int64_t n, const MgxCell *grid, const uint8_t *agents, const uint8_t *obs, const uint8_t *atlas,
               int32_t tile_size, uint8_t *frames, void *stream) {
    if (!spec || n < 0 || tile_size < 1 || tile_size > RENDER_MAX_TILE) return MGX_ERR_INVALID_ARGUMENT;
    const int W = spec->width, H = spec->height, A = spec->num_agents, v = spec->view_size;
    if (W < 3 || H < 3 || W > 255 || H > 255 || A < 1 || A > MGX_MAX_AGENTS || v < 3 || (v & 1) == 0) return MGX_ERR_INVALID_ARGUMENT;
    if (spec->cell_bytes < 0 || spec->cell_bytes > 3) return MGX_ERR_INVALID_ARGUMENT;
    const int cb = cell_bytes(spec->cell_bytes);
    if (n == 0) return MGX_OK;
    if (!grid || !agents || !atlas || !frames || (cb == 2 && misaligned(grid, 2))) return MGX_ERR_INVALID_ARGUMENT;
    if (n * H > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const int T3 = 3 * tile_size, R = W * T3;
    const bool vec = tile_size % 4 == 0 && !misaligned(frames, 16) && !misaligned(atlas, 4);
    const char *stores = getenv("MGX_RENDER_STORES");
    const bool nt = !(stores && strcmp(stores, "plain") == 0);
    const uint32_t mT3 = recip32((uint32_t)T3);
    const float inv_R = 1.0f / (float)R;
    const auto *gp = reinterpret_cast<const uint8_t *>(grid);
    const dim3 blocks((unsigned)(n * H)), threads(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (cb == 1)
        hipLaunchKernelGGL(pick<1>(vec, nt), blocks, threads, 0, st, W, H, A, v, tile_size, gp, agents, obs, atlas, frames, mT3, inv_R);
    else if (cb == 3)
        hipLaunchKernelGGL(pick<3>(vec, nt), blocks, threads, 0, st, W, H, A, v, tile_size, gp, agents, obs, atlas, frames, mT3, inv_R);
    else
        hipLaunchKernelGGL(pick<2>(vec, nt), blocks, threads, 0, st, W, H, A, v, tile_size, gp, agents, obs, atlas, frames, mT3, inv_R);
    return finish_launch();
}

int mgx_render_atlas_planar(int32_t tile_size, uint8_t *atlas, void *stream) {
    if (tile_size < 1 || tile_size > RENDER_MAX_TILE || !atlas) return MGX_ERR_INVALID_ARGUMENT;
    const int total = RENDER_KEYS * tile_size * tile_size;
    hipLaunchKernelGGL(render_atlas_planar_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       tile_size, total, render_trig_host(), atlas);
    return finish_launch();
}

int mgx_render_views(const MgxSpec *spec, int64_t n_views, const uint8_t *obs, const uint8_t *dir, const uint8_t *color,
                     int64_t color_period, const uint8_t *atlas, int32_t tile_size, uint32_t flags, uint8_t *frames, void *stream) {
    if (!spec || n_views < 0 || tile_size < 1 || tile_size > RENDER_MAX_TILE || color_period < 1) return MGX_ERR_INVALID_ARGUMENT;
    if (flags & ~(uint32_t)(MGX_VIEWS_HIGHLIGHT | MGX_VIEWS_PLANAR)) return MGX_ERR_INVALID_ARGUMENT;
    const int v = spec->view_size, ts = tile_size;
    if (v < 3 || v > MGX_MAX_VIEW || (v & 1) == 0) return MGX_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return MGX_OK;
    if (!obs || !dir || !color || !atlas || !frames) return MGX_ERR_INVALID_ARGUMENT;
    ViewFrameGeom g;
    g.v = v; g.ts = ts; g.planar = (flags & MGX_VIEWS_PLANAR) ? 1 : 0;
    g.P = v * ts;
    g.U = g.planar ? ts : 3 * ts;
    g.R = v * g.U;
    g.NR = g.planar ? 3 * g.P : g.P;
    g.F = 3 * g.P * g.P;
    g.tile_bytes = 3 * ts * ts;
    g.inv_U = 1.0f / (float)g.U; g.inv_R = 1.0f / (float)g.R; g.inv_P = 1.0f / (float)g.P; g.inv_F = 1.0f / (float)g.F;
    g.inv_ts = 1.0f / (float)ts;
    const int G = views_per_group(g.F);
    const int64_t groups = (n_views + G - 1) / G;
    if (groups > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const bool vec = ts % 4 == 0 && !misaligned(frames, 16) && !misaligned(atlas, 4);
    const char *stores = getenv("MGX_RENDER_STORES");
    const bool nt = !(stores && strcmp(stores, "plain") == 0);
    auto kernel = vec ? (nt ? render_views_kernel<true, true> : render_views_kernel<true, false>) : render_views_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(256), 0, static_cast<hipStream_t>(stream), g, n_views, G,
                       (int)(flags & MGX_VIEWS_HIGHLIGHT), obs, dir, color, color_period, atlas, frames);
    return finish_launch();
}

}  // extern "C"
