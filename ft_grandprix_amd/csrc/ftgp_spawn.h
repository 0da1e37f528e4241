// ftgp_spawn.h -- the spawn rule (include/ftgp.h: ftgp_set_spawn_rule): the per-track start table, built on the host, and the draw of
// one car's start pose, shared by the HIP kernels and by the host harness (tools/spawn_check.cpp compiles exactly these functions for
// the CPU; tests/spawn_model.py restates them in numpy and the two are compared bit for bit).
//
// Every operation is binary64 with one rounding, written out one by one; the library is compiled with -ffp-contract=off.  The draw uses
// no trigonometry: the yaw offset enters as the tangent of its half, and the unit quaternion comes from one square root.
// (This file is not among the hashed kernel sources -- tools/evidence.py and bench.py keep one list --: after a change here alone,
// rebuild with __graft_entry__.build(force=True).)
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/ftgp.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef FTGP_HD
#if defined(__HIPCC__)
#define FTGP_HD __host__ __device__ __forceinline__
#else
#define FTGP_HD static inline
#endif
#endif

// the library's counter-based generator: spawn_mode 1's yaw jitter, FTGP_POLICY_RANDOM and the spawn rule
FTGP_HD uint64_t splitmix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
FTGP_HD double u01(uint64_t h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }
// an index in [0, n) from the upper half of a hash
FTGP_HD uint32_t ftgp_mul32(uint64_t h, int n) { return (uint32_t)(((h >> 32) * (uint64_t)n) >> 32); }

// ---------------------------------------------------------------------------------------------
// Spawn table (host): [FTGP_PATH_POINTS][4] x, y, qw, qz -- a car on path point p looks at point p + 1
static inline void ftgp_spawn_table(const FtgpTrack& t, double* spawn)
{
    for (int p = 0; p < FTGP_PATH_POINTS; ++p) {      // position_vehicles (custom.py:1240-1245) + euler_to_quaternion([angle, 0, 0]) (custom.py:81-87)
        const int p1 = (p + 1) % FTGP_PATH_POINTS;
        const double ang = atan2(t.path[2 * p1 + 1] - t.path[2 * p + 1], t.path[2 * p1] - t.path[2 * p]);
        spawn[4 * p] = t.path[2 * p]; spawn[4 * p + 1] = t.path[2 * p + 1]; spawn[4 * p + 2] = cos(ang / 2); spawn[4 * p + 3] = sin(ang / 2);
    }
}

// Start table (host): clear[p][side], side 0 = left, 1 = right -- how far a car may move sideways from path point p before it meets a
// wall pixel or the image's edge, in steps of half a pixel, looked no further than the off-track distance 1.0 (custom.py:1344).
//   spawn  [FTGP_PATH_POINTS][4] x, y, qw, qz (plan_track_tables)      clear  [FTGP_PATH_POINTS][2]
static inline bool ftgp_start_blocked(const FtgpTrack& t, double inv_px_x, double inv_px_y, double px, double py)
{
    const double u = (px - t.origin_x) * inv_px_x, w = (t.origin_y - py) * inv_px_y;      // the contact rows' look-up (include/ftgp.h)
    const double fu = floor(u), fw = floor(w);
    if (!(fu >= 0.0 && fu < (double)t.width && fw >= 0.0 && fw < (double)t.height)) return true;      // off the image
    const int ix = (int)fu, iy = (int)fw;
    return ((t.bits[(size_t)iy * t.words_per_row + (ix >> 5)] >> (ix & 31)) & 1u) != 0;
}

static inline void ftgp_start_table(const FtgpTrack& t, const double* spawn, double* clear)
{
    const double inv_px_x = 1.0 / t.px_size_x, inv_px_y = 1.0 / t.px_size_y;
    const double delta = 0.5 * (t.px_size_x < t.px_size_y ? t.px_size_x : t.px_size_y);
    const int K = (int)ceil(1.0 / delta);
    for (int p = 0; p < FTGP_PATH_POINTS; ++p) {
        const double X = spawn[4 * p], Y = spawn[4 * p + 1], qw = spawn[4 * p + 2], qz = spawn[4 * p + 3];
        const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
        for (int side = 0; side < 2; ++side) {
            const double nx = side == 0 ? -sh : sh, ny = side == 0 ? ch : -ch;      // left normal (-sh, ch), right its negation
            int m = K + 1;
            for (int k = 0; k <= K; ++k) {
                const double d = (double)k * delta;
                if (ftgp_start_blocked(t, inv_px_x, inv_px_y, X + d * nx, Y + d * ny)) { m = k; break; }
            }
            clear[2 * p + side] = delta * (double)(m - 1 > 0 ? m - 1 : 0);
        }
    }
}

// the ordered list of the window's points that pass the margin; returns their number
static inline int ftgp_start_list(const FtgpSpawnRule& r, const double* clear, int32_t* start)
{
    int n = 0;
    for (int i = 0; i < r.n_points; ++i) {
        const int p = (r.first_point + i) % FTGP_PATH_POINTS;
        if (clear[2 * p] < r.margin || clear[2 * p + 1] < r.margin) continue;
        start[n++] = p;
    }
    return n;
}

// ---------------------------------------------------------------------------------------------
// The draw.  The rule as the kernels read it, in device memory: they are handed its address, null while no rule is set.
struct FtgpSpawnDev {
    const int32_t* start;         // [n_tracks][FTGP_PATH_POINTS] the start points of every track, the first n_start[t] of a row
    const int32_t* n_start;       // [n_tracks]
    const double* clear;          // [n_tracks][FTGP_PATH_POINTS][2]
    int64_t* episodes;            // [n_envs] resets of every env since the rule was set
    double margin, lateral_frac, yaw_tan;
    int32_t shuffle_grid, pad;
};

struct FtgpSpawnPose {
    double x, y, qw, qz;
    int32_t p, slot, offset, pad; // path point, grid slot, nearest centre-line point of (x, y)
};

// Car `a` of an env of `c` cars, global env index G, episode k.  start / clear / spawn: the rows of the env's track.  The centre-line
// is read from the spawn table, whose x, y columns are the path points as they are: one table pointer less to carry.
FTGP_HD void ftgp_spawn_draw(uint64_t seed, uint64_t G, uint64_t k, int c, int a, const int32_t* start, int n_start, const double* clear,
                             const double* spawn, double margin, double lateral_frac, double yaw_tan, int shuffle_grid, FtgpSpawnPose& o)
{
    const uint64_t hE = splitmix64(splitmix64(seed ^ (0x5350574E52554C45ull + G)) ^ k);
    const int b = start[ftgp_mul32(hE, n_start)];
    // the grid: slot[i] = nibble i (cars_per_env <= 8), so that the shuffle indexes no array
    uint32_t grid = 0x76543210u;
    if (shuffle_grid) {
        uint64_t h = hE;
#pragma unroll 1
        for (int i = c - 1; i >= 1; --i) {
            h = splitmix64(h);
            const int j = (int)ftgp_mul32(h, i + 1);
            const uint32_t d = ((grid >> (4 * i)) ^ (grid >> (4 * j))) & 15u;
            grid ^= (d << (4 * i)) ^ (d << (4 * j));
        }
    }
    const int slot = (int)((grid >> (4 * a)) & 15u);
    const int p = (b + 2 * slot) % FTGP_PATH_POINTS;          // custom.py:1112: two path points between grid neighbours
    const uint64_t hC = splitmix64(hE ^ (0xD6E8FEB86659FD93ull * (uint64_t)(a + 1)));
    const double w = 2.0 * u01(hC) - 1.0;
    const double v = 2.0 * u01(splitmix64(hC)) - 1.0;
    const double qw = spawn[4 * p + 2], qz = spawn[4 * p + 3];
    const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
    // lateral offset: along the left normal (-sh, ch), within the room of the side it points to
    const double cl = clear[2 * p + (w >= 0.0 ? 0 : 1)] - margin;
    const double room = cl > 0.0 ? cl : 0.0;
    const double lat = (lateral_frac * w) * room;
    o.x = spawn[4 * p] + lat * (-sh);
    o.y = spawn[4 * p + 1] + lat * ch;
    // yaw: the rotation by 2 atan(t) as a quaternion, times the table's.  t == 0 (no jitter) leaves the table's quaternion as it is: its
    // norm is 1 only to within an ulp, and dividing by it would move a start without jitter off spawn_mode 0's by that ulp
    const double t = yaw_tan * v;
    o.qw = qw; o.qz = qz;
    if (t != 0.0) {
        const double n = sqrt(1.0 + t * t), cj = 1.0 / n, sj = t / n;
        const double nw = qw * cj - qz * sj, nz = qz * cj + qw * sj;
        const double m = sqrt(nw * nw + nz * nz);
        o.qw = nw / m; o.qz = nz / m;
    }
    // progress offset: the nearest centre-line point of the pose drawn (K3's arithmetic and its strict <)
    double best = 0.0; int closest = 0;
#pragma unroll 1
    for (int i = 0; i < FTGP_PATH_POINTS; ++i) {
        const double dx = spawn[4 * i] - o.x, dy = spawn[4 * i + 1] - o.y;
        const double d = dx * dx + dy * dy;
        if (i == 0 || d < best) { best = d; closest = i; }
    }
    o.p = p; o.slot = slot; o.offset = closest; o.pad = 0;
}
