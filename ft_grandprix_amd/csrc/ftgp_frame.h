// ftgp_frame.h -- the track frame (include/ftgp.h "Track frame", steps 1 - 6): the element operations of one row, shared by the HIP
// kernels -- ftgp_io_frame_kernel, the finish kernel's frame_row_lane, the rival search and the network driver's frame inputs
// (net_inputs) -- and by the host harness (tools/net_check.cpp compiles exactly these functions for the CPU; tests/frame_model.py
// restates the header's text in numpy and the two are compared bit for bit).
//
// Every operation is binary64 with one rounding, written out one by one; the library is compiled with -ffp-contract=off.  / and sqrt
// are IEEE.  Comparisons are written as comparisons: what a NaN does is part of the text.  An entry is rounded once to binary32.
// (This file is not among the hashed kernel sources, as ftgp_net.h: after a change here alone, rebuild with
// __graft_entry__.build(force=True).)
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

// step 1, one candidate: the progress block's expression (K3)
FTGP_HD double frame_dist2(const double* __restrict__ path, int i, double x, double y)
{
    const double dx = path[2 * i] - x, dy = path[2 * i + 1] - y;
    return dx * dx + dy * dy;
}
// the total order the lanes of a search fold with: the smaller d, on equal d the smaller index -- the first minimum.  A NaN never wins.
FTGP_HD bool frame_nearer(double od, int oi, double d, int i) { return od < d || (od == d && oi < i); }

// step 2 of the row: the pose projected on segment a -> a + 1
struct FrameSeg { double ex, ey, L2, rx, ry, t, g2; };
FTGP_HD FrameSeg frame_segment(const double* __restrict__ path, int a, double x, double y)
{
    const int b = a + 1 < FTGP_PATH_POINTS ? a + 1 : 0;
    const double xa = path[2 * a], ya = path[2 * a + 1];
    FrameSeg g;
    g.ex = path[2 * b] - xa; g.ey = path[2 * b + 1] - ya;
    g.L2 = g.ex * g.ex + g.ey * g.ey;
    g.rx = x - xa; g.ry = y - ya;
    if (g.L2 == 0.0) { g.ex = 1.0; g.ey = 0.0; g.L2 = 1.0; g.t = 0.0; }
    else {
        const double t = (g.rx * g.ex + g.ry * g.ey) / g.L2;
        g.t = t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t;
    }
    const double fx = xa + g.t * g.ex, fy = ya + g.t * g.ey;
    const double gx = x - fx, gy = y - fy;
    g.g2 = gx * gx + gy * gy;
    return g;
}

// step 5: fixed entry k of the segment taken; s comes back unrounded.  One numerator and one denominator per entry, so that a caller
// with k in a register (the network driver: lane k forms entry k) runs one division for all four
struct FrameFixed { float x, y, z, w; };
FTGP_HD float frame_fixed_entry(const FrameSeg& g, int a, double ch, double sh, int k, double& s_out)
{
    const double len = sqrt(g.L2);
    double s = (double)a + g.t;
    if (s >= 100.0) s = s - 100.0;
    s_out = s;
    const double num = k == 0 ? g.ex * g.ry - g.ey * g.rx : k == 1 ? g.ex * ch + g.ey * sh : k == 2 ? g.ey * ch - g.ex * sh : s;
    const double den = k == 3 ? 100.0 : len;
    return (float)(num / den);
}
FTGP_HD FrameFixed frame_fixed(const FrameSeg& g, int a, double ch, double sh, double& s_out)
{
    FrameFixed f;
    f.x = frame_fixed_entry(g, a, ch, sh, 0, s_out); f.y = frame_fixed_entry(g, a, ch, sh, 1, s_out); f.z = frame_fixed_entry(g, a, ch, sh, 2, s_out);
    f.w = frame_fixed_entry(g, a, ch, sh, 3, s_out);
    return f;
}

// step 6: look-ahead point k behind segment a
struct FramePoint { float x, y; };
FTGP_HD FramePoint frame_ahead(const double* __restrict__ path, int a, int k, int stride, double x, double y, double ch, double sh)
{
    const int q = (a + 1 + k * stride) % FTGP_PATH_POINTS;
    const double dx = path[2 * q] - x, dy = path[2 * q + 1] - y;
    FramePoint p;
    p.x = (float)(dx * ch + dy * sh); p.y = (float)(dy * ch - dx * sh);
    return p;
}

// The whole row by one thread: the search as the progress block runs it, then steps 2 - 6 (the finish kernel at the spawn pose of an env
// it has just reset; the host harness)
FTGP_HD void frame_row(const double* __restrict__ path, double x, double y, double qw, double qz, int n_ahead, int stride, float* __restrict__ o)
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
    const double ch = qw * qw - qz * qz, sh = 2.0 * (qw * qz);
    double s;
    const FrameFixed f = frame_fixed(g, seg, ch, sh, s);
    o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = f.w;
#if defined(__HIP_DEVICE_COMPILE__)
    #pragma unroll 1
#endif
    for (int k = 0; k < n_ahead; ++k) {
        const FramePoint p = frame_ahead(path, seg, k, stride, x, y, ch, sh);
        o[FTGP_FRAME_FIXED + 2 * k] = p.x; o[FTGP_FRAME_FIXED + 2 * k + 1] = p.y;
    }
}
