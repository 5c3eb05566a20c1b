// mgx_render.h -- one tile of the reference's frame, evaluated per pixel: Grid.render_tile (multigrid/core/grid.py:198-254) for
// every key, bit for bit.
//
// A frame (MultiGridEnv.get_full_render, multigrid/base.py:707-760) is a grid of tiles, and a tile depends only on a small key:
// the cell's appearance (what its (type, color, state) draws), the agent drawn over it (colour and direction, or none) and
// whether it is highlighted.  There are RENDER_APPEARANCES * RENDER_OVERLAYS * 2 = 2 500 keys.  libmgx.so renders each of them
// once into an atlas on the device (mgx_render_atlas) and blits atlas rows into the frames (mgx_render); compiled by g++, the
// same functions build the atlas on the host for the CPU tests.
//
// The reference draws a tile at 3x the size (subdivs = 3), then takes 3x3 means (utils/rendering.py: downsample).  Every
// supersampled pixel is a uint8 colour decided by the filter functions of utils/rendering.py in the order the render methods call
// them (a later fill overwrites an earlier one).  What decides exactness, mirrored here:
//   * pixel centres are float64, ((x + 0.5) / S);
//   * point_in_rect / point_in_circle are plain float64 compares and sums;
//   * point_in_triangle and point_in_line keep their vertices / end points as float32 arrays and the query point as float64, so
//     under NumPy's promotion rules (NEP 50) dot00, dot01, dot11, the line's direction and its length are float32; dot02, dot12,
//     the projection and the distance are float64, and NumPy's 2-element float64 dot is fma(x1, y1, x0 * y0) -- written here with
//     an explicit fma (the file is compiled with -ffp-contract=off, so nothing else is contracted);
//   * rotate_fn takes cos(-theta) and sin(-theta) from the host's libm: the caller passes them (RenderTrig), never device cos;
//   * Floor's rgb() / 2 and the locked door's 0.45 * c are float colours truncated into the uint8 image; highlight_img is
//     img + 0.3 * (255 - img) in float64, clipped, truncated, at the supersampled level;
//   * downsample returns float64 means, ((a + b) + c) / 3 over x, then over y; Grid.render truncates them to uint8.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <math.h>
#include <stdint.h>
#endif

#if defined(__HIPCC__)
#define MGX_RHD __host__ __device__ __forceinline__
#else
#define MGX_RHD inline
#endif

namespace mgx {

// appearances: 0 empty | 1-6 wall (and goal) by colour | 7-12 floor | 13-30 door, 3 * colour + state | 31-36 key | 37-42 ball |
// 43-48 box | 49 lava.  Overlays: 0 none | 1 + 4 * colour + dir = a live agent.
enum : int { RA_EMPTY = 0, RA_WALL = 1, RA_FLOOR = 7, RA_DOOR = 13, RA_KEY = 31, RA_BALL = 37, RA_BOX = 43, RA_LAVA = 49 };
constexpr int RENDER_APPEARANCES = 50;
constexpr int RENDER_OVERLAYS = 25;
constexpr int RENDER_KEYS = RENDER_APPEARANCES * RENDER_OVERLAYS * 2;
constexpr int RENDER_MAX_TILE = 64;

// cos(-theta), sin(-theta) of theta = 0.5 * pi * dir (multigrid/core/agent.py:165), dir = 0..3
struct RenderTrig {
    double c[4], s[4];
};

#if !defined(__HIPCC_RTC__)
// host only: the values Python's math.cos / math.sin give (both call the C library)
inline RenderTrig render_trig_host() {
    RenderTrig t;
    for (int d = 0; d < 4; d++) {
        volatile double theta = 0.5 * 3.141592653589793 * d;      // (np.pi; volatile: no compile-time folding of cos / sin)
        t.c[d] = cos(-theta);
        t.s[d] = sin(-theta);
    }
    return t;
}
#endif

// The appearance of a cell (type, color, state) as the reference draws it: Grid.get decodes it (WorldObj.from_array) and
// render_tile draws the object.  A goal draws the same tile as a wall of its colour (world_object.py Goal.render / Wall.render),
// lava ignores its colour, a box draws a plain box whatever it holds (only state & 3 is a state; a box's content rides in the
// upper bits).  Empty, unseen, agent and anything out of range (type > 10, colour > 5, door state 3) draw no object.
MGX_RHD int render_appearance(uint32_t t, uint32_t c, uint32_t s) {
    s &= 3u;
    if (t == 9u) return RA_LAVA;
    if (c > 5u) return RA_EMPTY;
    switch (t) {
    case 2u: case 8u: return RA_WALL + (int)c;
    case 3u: return RA_FLOOR + (int)c;
    case 4u: return s <= 2u ? RA_DOOR + 3 * (int)c + (int)s : RA_EMPTY;
    case 5u: return RA_KEY + (int)c;
    case 6u: return RA_BALL + (int)c;
    case 7u: return RA_BOX + (int)c;
    default: return RA_EMPTY;
    }
}

// the atlas index of a key
MGX_RHD int render_key(int appearance, int overlay, int highlight) { return (appearance * RENDER_OVERLAYS + overlay) * 2 + highlight; }

// The key of one cell of an agent's VIEW drawn as the viewer sees it (include/mgx.h "VIEW FRAMES"): cell bytes (t, c, s) of
// image[i, j], `own` = the viewer's cell (v / 2, v - 1).  The viewer faces up in its view (direction 3), so another agent -- a
// cell of type `agent` (10) whose state byte is its world direction -- is turned by the viewer's direction: (s - dir + 3) & 3,
// over the empty tile (the observation does not say what lies under it).  The viewer's own cell holds what it carries
// (utils/obs.py:204-207) and always draws the viewer; a colour above 5 has no overlay, as in the full frame.  Highlighting
// (MiniGrid's POV convention) shades every cell that is not `unseen`; an unseen cell draws the plain empty tile.  Any bytes are
// legal: only dir & 3 counts, and the key is below RENDER_KEYS for every input.
MGX_RHD int render_view_key(uint32_t t, uint32_t c, uint32_t s, bool own, uint32_t viewer_dir, uint32_t viewer_color, bool highlight) {
    int ov = 0;
    if (own)
        ov = viewer_color <= 5u ? 1 + 4 * (int)viewer_color + 3 : 0;
    else if (t == 10u && c <= 5u)
        ov = 1 + 4 * (int)c + (int)((s - viewer_dir + 3u) & 3u);
    return render_key(render_appearance(t, c, s), ov, highlight && t != 0u ? 1 : 0);
}

// multigrid/core/constants.py:12-19 COLORS
MGX_RHD uint32_t render_rgb(int color) {
    switch (color) {
    case 0: return 0x0000ffu;            // red     (255, 0, 0)   packed r | g << 8 | b << 16
    case 1: return 0x00ff00u;            // green   (0, 255, 0)
    case 2: return 0xff0000u;            // blue    (0, 0, 255)
    case 3: return 0xc32770u;            // purple  (112, 39, 195)
    case 4: return 0x00ffffu;            // yellow  (255, 255, 0)
    default: return 0x646464u;           // grey    (100, 100, 100)
    }
}
// a float colour k * rgb, truncated into the uint8 image (Floor: rgb() / 2; locked door: 0.45 * c)
MGX_RHD uint32_t render_scaled(uint32_t rgb, double k, bool halve) {
    uint32_t out = 0;
    for (int ch = 0; ch < 3; ch++) {
        const double v = (double)((rgb >> (8 * ch)) & 0xffu);
        out |= (uint32_t)(halve ? v / 2.0 : k * v) << (8 * ch);
    }
    return out;
}

// utils/rendering.py filter functions
MGX_RHD bool in_rect(double x, double y, double xmin, double xmax, double ymin, double ymax) {
    return x >= xmin && x <= xmax && y >= ymin && y <= ymax;
}
MGX_RHD bool in_circle(double x, double y, double cx, double cy, double r) {
    return (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r * r;
}
MGX_RHD bool in_line(double x, double y, double x0, double y0, double x1, double y1, double r) {
    const double xmin = (x0 < x1 ? x0 : x1) - r, xmax = (x0 > x1 ? x0 : x1) + r;     // python min / max of the float64 arguments
    const double ymin = (y0 < y1 ? y0 : y1) - r, ymax = (y0 > y1 ? y0 : y1) + r;
    if (x < xmin || x > xmax || y < ymin || y > ymax) return false;
    const float p0x = (float)x0, p0y = (float)y0;
    const float dx = (float)x1 - p0x, dy = (float)y1 - p0y;                           // float32 arrays
    const float dist = sqrtf(dx * dx + dy * dy);                                      // np.linalg.norm of float32
    const float ux = dx / dist, uy = dy / dist;
    const double qx = x - (double)p0x, qy = y - (double)p0y;                          // float64 query point
    double a = fma(qy, (double)uy, qx * (double)ux);                                  // np.dot, float64
    a = a > 0.0 ? a : 0.0;                                                            // np.clip(a, 0, dist)
    a = a < (double)dist ? a : (double)dist;
    const double px = (double)p0x + a * (double)ux, py = (double)p0y + a * (double)uy;
    const double ex = x - px, ey = y - py;
    return sqrt(fma(ey, ey, ex * ex)) <= r;                                           // np.linalg.norm of float64
}
// the agent's triangle (0.12, 0.19), (0.87, 0.50), (0.12, 0.81), rotated about (0.5, 0.5) (agent.py:150-167)
MGX_RHD bool in_agent(double x, double y, double cs, double sn) {
    const double xr = x - 0.5, yr = y - 0.5;
    const double x2 = 0.5 + xr * cs - yr * sn;                                        // rotate_fn
    const double y2 = 0.5 + yr * cs + xr * sn;
    const float ax = 0.12f, ay = 0.19f, bx = 0.87f, by = 0.50f, cx = 0.12f, cy = 0.81f;
    const float v0x = cx - ax, v0y = cy - ay, v1x = bx - ax, v1y = by - ay;
    const double v2x = x2 - (double)ax, v2y = y2 - (double)ay;
    const float dot00 = v0x * v0x + v0y * v0y;
    const float dot01 = v0x * v1x + v0y * v1y;
    const float dot11 = v1x * v1x + v1y * v1y;
    const double dot02 = fma((double)v0y, v2y, (double)v0x * v2x);
    const double dot12 = fma((double)v1y, v2y, (double)v1x * v2x);
    const float inv_denom = 1.0f / (dot00 * dot11 - dot01 * dot01);
    const double u = ((double)dot11 * dot02 - (double)dot01 * dot12) * (double)inv_denom;
    const double v = ((double)dot00 * dot12 - (double)dot01 * dot02) * (double)inv_denom;
    return u >= 0.0 && v >= 0.0 && (u + v) < 1.0;
}

// The colour (r | g << 8 | b << 16) of supersampled pixel (px, py) of an S x S tile image (S = 3 * tile_size).
MGX_RHD uint32_t render_subpixel(int appearance, int overlay, int highlight, int px, int py, int S, const RenderTrig &trig) {
    const double x = ((double)px + 0.5) / (double)S, y = ((double)py + 0.5) / (double)S;
    const uint32_t kBlack = 0u, kGrey = 0x646464u;
    uint32_t col = kBlack;
    // grid lines (top and left edges)
    if (in_rect(x, y, 0, 0.031, 0, 1)) col = kGrey;
    if (in_rect(x, y, 0, 1, 0, 0.031)) col = kGrey;
    const int a = appearance;
    if (a >= RA_WALL && a < RA_FLOOR) {                                  // Wall / Goal
        col = render_rgb(a - RA_WALL);
    } else if (a >= RA_FLOOR && a < RA_DOOR) {                           // Floor
        if (in_rect(x, y, 0.031, 1, 0.031, 1)) col = render_scaled(render_rgb(a - RA_FLOOR), 0.0, true);
    } else if (a >= RA_DOOR && a < RA_KEY) {                             // Door
        const int k = a - RA_DOOR, st = k % 3;
        const uint32_t c = render_rgb(k / 3);
        if (st == 0) {                                                   // open
            if (in_rect(x, y, 0.88, 1.00, 0.00, 1.00)) col = c;
            if (in_rect(x, y, 0.92, 0.96, 0.04, 0.96)) col = kBlack;
        } else if (st == 2) {                                            // locked
            col = c;
            if (in_rect(x, y, 0.06, 0.94, 0.06, 0.94)) col = render_scaled(c, 0.45, false);
            if (in_rect(x, y, 0.52, 0.75, 0.50, 0.56)) col = c;
        } else {                                                         // closed
            col = c;
            if (in_rect(x, y, 0.04, 0.96, 0.04, 0.96)) col = kBlack;
            if (in_rect(x, y, 0.08, 0.92, 0.08, 0.92)) col = c;
            if (in_rect(x, y, 0.12, 0.88, 0.12, 0.88)) col = kBlack;
            if (in_circle(x, y, 0.75, 0.50, 0.08)) col = c;
        }
    } else if (a >= RA_KEY && a < RA_BALL) {                             // Key
        const uint32_t c = render_rgb(a - RA_KEY);
        if (in_rect(x, y, 0.50, 0.63, 0.31, 0.88)) col = c;
        if (in_rect(x, y, 0.38, 0.50, 0.59, 0.66)) col = c;
        if (in_rect(x, y, 0.38, 0.50, 0.81, 0.88)) col = c;
        if (in_circle(x, y, 0.56, 0.28, 0.190)) col = c;
        if (in_circle(x, y, 0.56, 0.28, 0.064)) col = kBlack;
    } else if (a >= RA_BALL && a < RA_BOX) {                             // Ball
        if (in_circle(x, y, 0.5, 0.5, 0.31)) col = render_rgb(a - RA_BALL);
    } else if (a >= RA_BOX && a < RA_LAVA) {                             // Box
        const uint32_t c = render_rgb(a - RA_BOX);
        if (in_rect(x, y, 0.12, 0.88, 0.12, 0.88)) col = c;
        if (in_rect(x, y, 0.18, 0.82, 0.18, 0.82)) col = kBlack;
        if (in_rect(x, y, 0.16, 0.84, 0.47, 0.53)) col = c;
    } else if (a == RA_LAVA) {                                           // Lava
        col = 0x0080ffu;                                                 // (255, 128, 0)
        for (int i = 0; i < 3; i++) {
            const double ylo = 0.3 + 0.2 * i, yhi = 0.4 + 0.2 * i;
            if (in_line(x, y, 0.1, ylo, 0.3, yhi, 0.03)) col = kBlack;
            if (in_line(x, y, 0.3, yhi, 0.5, ylo, 0.03)) col = kBlack;
            if (in_line(x, y, 0.5, ylo, 0.7, yhi, 0.03)) col = kBlack;
            if (in_line(x, y, 0.7, yhi, 0.9, ylo, 0.03)) col = kBlack;
        }
    }
    if (overlay > 0) {                                                   // a live agent
        const int d = (overlay - 1) & 3;
        if (in_agent(x, y, trig.c[d], trig.s[d])) col = render_rgb((overlay - 1) >> 2);
    }
    if (highlight) {                                                     // highlight_img
        uint32_t out = 0;
        for (int ch = 0; ch < 3; ch++) {
            const uint32_t v = (col >> (8 * ch)) & 0xffu;
            double b = (double)v + 0.3 * (double)(255u - v);
            b = b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b);
            out |= (uint32_t)b << (8 * ch);
        }
        col = out;
    }
    return col;
}

// Output pixel (ox, oy) of a tile of `tile_size` pixels: the 3x3 means of downsample, truncated to uint8 as Grid.render stores
// them; r | g << 8 | b << 16.
MGX_RHD uint32_t render_pixel(int appearance, int overlay, int highlight, int ox, int oy, int tile_size, const RenderTrig &trig) {
    const int S = 3 * tile_size;
    uint32_t sub[3][3];
    for (int dy = 0; dy < 3; dy++)
        for (int dx = 0; dx < 3; dx++)
            sub[dy][dx] = render_subpixel(appearance, overlay, highlight, 3 * ox + dx, 3 * oy + dy, S, trig);
    uint32_t out = 0;
    for (int ch = 0; ch < 3; ch++) {
        double m[3];
        for (int dy = 0; dy < 3; dy++) {
            const double s = ((double)((sub[dy][0] >> (8 * ch)) & 0xffu) + (double)((sub[dy][1] >> (8 * ch)) & 0xffu))
                             + (double)((sub[dy][2] >> (8 * ch)) & 0xffu);
            m[dy] = s / 3.0;                                             // mean over x (axis 3)
        }
        const double v = ((m[0] + m[1]) + m[2]) / 3.0;                   // mean over y (axis 1)
        out |= (uint32_t)v << (8 * ch);
    }
    return out;
}

// A whole tile, u8[tile_size, tile_size, 3] at `out` (the host build of the atlas; the device kernel runs render_pixel per lane).
inline void render_tile(int key, int tile_size, const RenderTrig &trig, uint8_t *out) {
    const int hl = key & 1, ov = (key >> 1) % RENDER_OVERLAYS, ap = (key >> 1) / RENDER_OVERLAYS;
    for (int oy = 0; oy < tile_size; oy++)
        for (int ox = 0; ox < tile_size; ox++) {
            const uint32_t c = render_pixel(ap, ov, hl, ox, oy, tile_size, trig);
            uint8_t *p = out + 3 * (oy * tile_size + ox);
            p[0] = (uint8_t)c; p[1] = (uint8_t)(c >> 8); p[2] = (uint8_t)(c >> 16);
        }
}

}  // namespace mgx
