// ftgp_rival.h -- the rival row (include/ftgp.h "Rival rows of the device step", steps 1 - 4): the element operations of one row, shared
// by the HIP kernels -- ftgp_io_rival_kernel, the finish kernel's rows at the spawn state (rival_lds_put, rival_row_lane), the network
// driver's rival inputs (net_inputs) -- and by the host harness (tools/net_check.cpp --rivals compiles exactly these functions for the
// CPU; tests/rival_model.py restates the header's text in numpy and the two are compared bit for bit).
//
// The rules are ftgp_frame.h's: every operation is binary64 with one rounding, written out one by one (-ffp-contract=off); comparisons
// are written as comparisons, so what a NaN does is part of the text; an entry is rounded once to binary32.
// (This file is not among the hashed kernel sources, as ftgp_frame.h: after a change here alone, rebuild with
// __graft_entry__.build(force=True).)
#pragma once
#include "ftgp_frame.h"

// step 1: race progress from what the search found
FTGP_HD double rival_progress(int32_t abs_completion, double s, int c, bool off)
{
    double f = s - (double)c;
    if (f >= 50.0) f = f - 100.0;
    if (f < -50.0) f = f + 100.0;
    if (off) f = 0.0;
    return (double)abs_completion + f;
}

// step 2: is car b (slot b) ahead of car a (slot a)?
FTGP_HD bool rival_ahead(bool fin_b, int64_t fs_b, double g_b, int b, bool fin_a, int64_t fs_a, double g_a, int a)
{
    if (fin_b && fin_a) return fs_b < fs_a || (fs_b == fs_a && b < a);
    if (fin_b) return true;
    if (fin_a) return false;
    return g_b > g_a || (g_b == g_a && b < a);
}

// what a mate slot needs of a car: the pose, the heading (ch, sh) of step 4, the velocity and the unrounded s of the frame row
struct RivalCar { double x, y, ch, sh, vx, vy, s; };
FTGP_HD RivalCar rival_car(double x, double y, double qw, double qz, double vx, double vy, double s)
{
    RivalCar k;
    k.x = x; k.y = y; k.ch = qw * qw - qz * qz; k.sh = 2.0 * (qw * qz); k.vx = vx; k.vy = vy; k.s = s;
    return k;
}

// step 4: entry q of mate b in a's slot.  Entries 0 - 5 are three pairs (u, v) -- the position, the heading, the velocity of b relative to
// a -- turned into a's frame: the even one u*ch + v*sh, the odd one v*ch - u*sh; a caller with q in a register (the network driver: lane
// q of a mate forms entry q) runs one pair of products for all six.
FTGP_HD float rival_mate_entry(const RivalCar& a, const RivalCar& b, int q)
{
    if (q == 7) return 1.0f;
    if (q == 6) {
        double tg = b.s - a.s;
        if (tg >= 50.0) tg = tg - 100.0;
        if (tg < -50.0) tg = tg + 100.0;
        return (float)tg;
    }
    const int p = q >> 1;
    const double u = p == 0 ? b.x - a.x : p == 1 ? b.ch : b.vx - a.vx;
    const double v = p == 0 ? b.y - a.y : p == 1 ? b.sh : b.vy - a.vy;
    return (q & 1) ? (float)(v * a.ch - u * a.sh) : (float)(u * a.ch + v * a.sh);
}
// ... and the eight of them
FTGP_HD void rival_mate(const RivalCar& a, const RivalCar& b, float* __restrict__ o)
{
#if defined(__HIP_DEVICE_COMPILE__)
    #pragma unroll
#endif
    for (int q = 0; q < FTGP_RIVAL_FLOATS; ++q) o[q] = rival_mate_entry(a, b, q);
}

// A car's place on the track, by one thread: the search as the progress block runs it, steps 2 and 3 of the frame row (s alone), step 1
// of the rival row.  abs_completion: column 3 of ftgp_get_progress.
FTGP_HD void rival_place(const double* __restrict__ path, double x, double y, int32_t abs_completion, double& s_out, double& g_out)
{
    double best = 0.0; int c = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    #pragma unroll 1
#endif
    for (int i = 0; i < FTGP_PATH_POINTS; ++i) {
        const double d = frame_dist2(path, i, x, y);
        if (i == 0 || d < best) { best = d; c = i; }
    }
    const int pa = c > 0 ? c - 1 : FTGP_PATH_POINTS - 1;
    FrameSeg g = frame_segment(path, c, x, y);
    int seg = c;
    {
        const FrameSeg ga = frame_segment(path, pa, x, y);
        if (ga.g2 < g.g2) { g = ga; seg = pa; }
    }
    double s = (double)seg + g.t;
    if (s >= 100.0) s = s - 100.0;
    s_out = s;
    g_out = rival_progress(abs_completion, s, c, best > 1.0);
}

// The whole row of the car in slot `slot` by one thread, from what every car of the env contributes (rival_car at rival_place's s, g,
// finish_step, finished): the operations of ftgp_io_rival_kernel on plain arrays of cpe entries.
FTGP_HD void rival_row(const RivalCar* __restrict__ car, const double* __restrict__ g, const int64_t* __restrict__ finish_step, const int32_t* __restrict__ finished,
                       int cpe, int slot, int n_rivals, float* __restrict__ o)
{
    const RivalCar a = car[slot];
    const double g_a = g[slot];
    const bool fin_a = finished[slot] != 0;
    const int64_t fs_a = finish_step[slot];
    int n_ahead = 0, n_racing = 0;
    double gap_ahead = INFINITY, gap_behind = INFINITY;
#if defined(__HIP_DEVICE_COMPILE__)
    #pragma unroll 1
#endif
    for (int b = 0; b < cpe; ++b) {
        const bool fin_b = finished[b] != 0;
        if (!fin_b) ++n_racing;
        if (b == slot) continue;
        const double g_b = g[b];
        const bool ahead = rival_ahead(fin_b, finish_step[b], g_b, b, fin_a, fs_a, g_a, slot);
        if (ahead) ++n_ahead;
        if (fin_b || fin_a) continue;
        const double gap = ahead ? g_b - g_a : g_a - g_b;
        if (ahead) { if (gap < gap_ahead) gap_ahead = gap; }
        else if (gap < gap_behind) gap_behind = gap;
    }
    o[0] = (float)(1 + n_ahead); o[1] = (float)n_racing;
    o[2] = gap_ahead == INFINITY ? 0.0f : (float)gap_ahead; o[3] = gap_behind == INFINITY ? 0.0f : (float)gap_behind;
    // the mates in (d2, slot) order: each turn takes the first one behind the last taken
    double last_d2 = -1.0; int last_b = -1;
#if defined(__HIP_DEVICE_COMPILE__)
    #pragma unroll 1
#endif
    for (int k = 0; k < n_rivals; ++k) {
        double best = 0.0; int bb = -1;
        if (!fin_a) {
#if defined(__HIP_DEVICE_COMPILE__)
            #pragma unroll 1
#endif
            for (int b = 0; b < cpe; ++b) {
                if (b == slot || finished[b]) continue;
                const double dx = car[b].x - a.x, dy = car[b].y - a.y;
                const double d2 = dx * dx + dy * dy;
                if (!(d2 > last_d2 || (d2 == last_d2 && b > last_b))) continue;      // taken already
                if (bb < 0 || d2 < best) { best = d2; bb = b; }
            }
        }
        float* m = o + FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * k;
        if (bb >= 0) { rival_mate(a, car[bb], m); last_d2 = best; last_b = bb; }
        else {
            for (int q = 0; q < FTGP_RIVAL_FLOATS; ++q) m[q] = 0.0f;
            last_d2 = INFINITY; last_b = FTGP_MAX_RIVALS + 1;      // nobody is left
        }
    }
}
