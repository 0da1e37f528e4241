// ftgp_net.h -- the network driver (include/ftgp.h: ftgp_set_net): the element operations of one evaluation, shared by the HIP kernels
// and by the host harness (tools/net_check.cpp compiles exactly these functions for the CPU; tests/net_model.py restates the header's
// text in numpy and the two are compared bit for bit) -- and of a collected decision (ftgp_collect_device: the mean, the noise, the clip and
// the guard; tools/collect_check.cpp and tests/collect_model.py likewise).
//
// Every operation is binary32 with one rounding, written out one by one; the library is compiled with -ffp-contract=off, and fmaf is
// written where a fused multiply-add is specified.  Comparisons are written as comparisons (no fminf / fmaxf): what a NaN does is then
// part of the text.  The state inputs are binary64, rounded once.
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

// ---- scan input ----
// a range as it enters a beam's minimum: no hit (< 0) = M, a hit = min(r, M)
FTGP_HD float ftgp_net_ray(float r, float M) { return r < 0.0f ? M : (r < M ? r : M); }
// the running minimum: the first of equal values stays
FTGP_HD float ftgp_net_min(float m, float v) { return v < m ? v : m; }
// the beam over `pool` consecutive ranges, scaled by inv = float32(1) / float32(M)
FTGP_HD float ftgp_net_beam(const float* r, int pool, float M, float inv)
{
    float m = ftgp_net_ray(r[0], M);
    for (int p = 1; p < pool; ++p) m = ftgp_net_min(m, ftgp_net_ray(r[p], M));
    return m * inv;
}

// ---- state inputs: entries 0 - 4 of the state row (ftgp_state_device), binary64 rounded once ----
FTGP_HD float ftgp_net_state(int i, double qw, double qz, double vx, double vy, double wz, double u_speed, double u_steer)
{
    const double c = qw * qw - qz * qz, s = 2.0 * (qw * qz);
    switch (i) {
    case 0: return (float)(vx * c + vy * s);
    case 1: return (float)(vy * c - vx * s);
    case 2: return (float)wz;
    case 3: return (float)u_speed;
    default: return (float)u_steer;
    }
}

// ---- activations ----
FTGP_HD float ftgp_net_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }      // a NaN stays a NaN
FTGP_HD float ftgp_net_relu(float a) { return a > 0.0f ? a : 0.0f; }                                       // a NaN gives 0
// Lambert's continued fraction of tanh, twelve levels, from the inside out
FTGP_HD float ftgp_net_tanh(float a)
{
    const float x = ftgp_net_clamp(a, -9.0f, 9.0f);
    const float x2 = x * x;
    float d = 25.0f;
    for (int k = 11; k >= 0; --k) d = (float)(2 * k + 1) + x2 / d;
    return ftgp_net_clamp(x / d, -1.0f, 1.0f);
}
FTGP_HD float ftgp_net_act(int act, float a)
{
    return act == FTGP_ACT_TANH ? ftgp_net_tanh(a) : act == FTGP_ACT_RELU ? ftgp_net_relu(a) : a;
}

// ---- controls: the output map and its guard ----
FTGP_HD void ftgp_net_controls(float y0, float y1, const float* scale, const float* offset, double* u_speed, double* u_steer)
{
    const float a = fmaf(y0, scale[0], offset[0]), b = fmaf(y1, scale[1], offset[1]);
    const bool ok = (a - a == 0.0f) && (b - b == 0.0f);          // both finite
    *u_speed = ok ? (double)a : 0.0;
    *u_steer = ok ? (double)b : 0.0;
}

// ---- collected actions (include/ftgp.h "Collected rollouts", step 1): the mean, the noise, the clip and the guard, one element each
// (tools/collect_check.cpp compiles these for the CPU; tests/collect_model.py restates the header's text)
FTGP_HD float ftgp_net_mean(float y, float scale, float offset) { return fmaf(y, scale, offset); }          // not guarded: a diverged network shows
FTGP_HD float ftgp_net_noisy(float m, float std, float noise) { return fmaf(std, noise, m); }               // 0 * inf = NaN: the guard's business
FTGP_HD float ftgp_net_clip(float a, float lo, float hi) { return a < lo ? lo : (a > hi ? hi : a); }        // a NaN stays a NaN
FTGP_HD bool ftgp_net_finite(float a) { return a - a == 0.0f; }
// the guard: both components, or neither
FTGP_HD float ftgp_net_guarded(float a, bool both_finite) { return both_finite ? a : 0.0f; }

// ---- collected values (include/ftgp.h "Collected rollouts with values"): the value element and one element step of the advantage scan
// (tools/collect_values_check.cpp compiles these for the CPU; tests/collect_values_model.py restates the header's text)
FTGP_HD float ftgp_net_value(float y, float scale, float offset) { return fmaf(y, scale, offset); }          // no guard: a diverged critic shows
// the advantage at t from the one at t + 1 (a_next; not looked at where last, term or trunc); gl = gamma * lam, rounded once on the host
FTGP_HD float ftgp_gae_step(float gamma, float gl, float reward, float value, float next_value, bool term, bool trunc, bool last, float a_next)
{
    const float nv = term ? 0.0f : next_value;
    const float d = fmaf(gamma, nv, reward) - value;
    return (last || term || trunc) ? d : fmaf(gl, a_next, d);
}
FTGP_HD float ftgp_gae_return(float advantage, float value) { return advantage + value; }

// ---- training (include/ftgp.h "Training on the device"): the scalars of one Adam step and its element step
// (tools/train_check.cpp compiles these for the CPU; tests/train_model.py restates the header's text)
// out = b1, b2, 1 - b1, 1 - b2, a = lr / (1 - beta1^t), r = 1 / sqrt(1 - beta2^t): binary64 (libm's pow and sqrt), each rounded once
static inline void ftgp_adam_scalars(float beta1, float beta2, float lr, int64_t t, float out[6])
{
    const double b1 = (double)beta1, b2 = (double)beta2;
    out[0] = beta1; out[1] = beta2;
    out[2] = (float)(1.0 - b1); out[3] = (float)(1.0 - b2);
    out[4] = (float)((double)lr / (1.0 - pow(b1, (double)t)));
    out[5] = (float)(1.0 / sqrt(1.0 - pow(b2, (double)t)));
}
// one parameter: torch's Adam without weight decay; sqrtf and / are IEEE
FTGP_HD void ftgp_adam_step(float* p, float* m, float* v, float g, float b1, float b2, float omb1, float omb2, float a, float r, float eps)
{
    const float m1 = fmaf(b1, *m, omb1 * g);
    const float v1 = fmaf(b2, *v, omb2 * (g * g));
    const float d = fmaf(sqrtf(v1), r, eps);
    *p = fmaf(-a, m1 / d, *p);
    *m = m1; *v = v1;
}

// ---- shapes: what ftgp_set_net checks, and the sizes that follow from a description ----
FTGP_HD int ftgp_net_inputs(const FtgpNetDesc* d) { return d->n_beams + (d->use_state ? FTGP_NET_STATE_INPUTS : 0); }
// the frame entries behind them (ftgp_set_net_frame): none without the struct or with enabled == 0
FTGP_HD int ftgp_net_frame_inputs(const FtgpNetFrame* f) { return (f && f->enabled) ? FTGP_FRAME_FIXED + 2 * f->n_ahead : 0; }
// ... and the rival entries behind those (ftgp_set_net_rivals): none without the struct or with enabled == 0
FTGP_HD int ftgp_net_rival_inputs(const FtgpNetRivals* r) { return (r && r->enabled) ? FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * r->n_rivals : 0; }
// number of binary32 parameters in the caller's layout: per layer W[n_out][n_in], then b[n_out]
FTGP_HD size_t ftgp_net_param_count(const FtgpNetDesc* d)
{
    size_t n = 0;
    int n_in = ftgp_net_inputs(d);
    for (int l = 0; l < d->n_layers; ++l) { n += (size_t)d->width[l] * (size_t)n_in + (size_t)d->width[l]; n_in = d->width[l]; }
    return n;
}

// ---- the library's layout of a parameter set, and of a population of them (ftgp_set_net_population) ----
// width[0] = n_in, width[l + 1] = outputs of layer l.  Per layer the weights transposed and padded, Wt[n_in][ld] with ld = n_out rounded
// up to 64, then b[ld]; the padding is zeros.  (tools/net_layout_check.cpp compiles these for the CPU; tests/test_net_population.py
// compares them with numpy.)
FTGP_HD int ftgp_net_ld(int n_out) { return (n_out + 63) & ~63; }
// floats of one set in the caller's layout and in the library's
FTGP_HD int ftgp_net_caller_floats(int n_layers, const int32_t* width)
{
    int n = 0;
    for (int l = 0; l < n_layers; ++l) n += width[l + 1] * width[l] + width[l + 1];
    return n;
}
FTGP_HD int ftgp_net_library_floats(int n_layers, const int32_t* width)
{
    int n = 0;
    for (int l = 0; l < n_layers; ++l) n += (width[l] + 1) * ftgp_net_ld(width[l + 1]);
    return n;
}
// where float i of the caller's layout (per layer W[n_out][n_in], then b[n_out]) sits in the library's; -1 past the last one
FTGP_HD int ftgp_net_library_index(int n_layers, const int32_t* width, int i)
{
    int o = 0;
    if (i < 0) return -1;
    for (int l = 0; l < n_layers; ++l) {
        const int n_in = width[l], n_out = width[l + 1], ld = ftgp_net_ld(n_out);
        if (i < n_in * n_out) return o + (i % n_in) * ld + i / n_in;
        i -= n_in * n_out; o += n_in * ld;
        if (i < n_out) return o + i;
        i -= n_out; o += ld;
    }
    return -1;
}
// floats from one member of a population to the next: the library's floats rounded up to 64, a whole 256-byte segment
FTGP_HD int ftgp_net_member_stride(int n_floats) { return (n_floats + 63) & ~63; }
// n_members sets, member after member in the caller's layout, into the library's at img -- [n_members] sets ftgp_net_member_stride
// apart, zeroed by the caller: only the parameters are written, the padding stays -- and back
FTGP_HD void ftgp_net_population_to_library(int n_layers, const int32_t* width, int n_members, const float* src, float* img)
{
    const int count = ftgp_net_caller_floats(n_layers, width);
    const size_t stride = (size_t)ftgp_net_member_stride(ftgp_net_library_floats(n_layers, width));
    for (size_t m = 0; m < (size_t)n_members; ++m)
        for (int i = 0; i < count; ++i) img[m * stride + (size_t)ftgp_net_library_index(n_layers, width, i)] = src[m * (size_t)count + (size_t)i];
}
FTGP_HD void ftgp_net_population_from_library(int n_layers, const int32_t* width, int n_members, const float* img, float* dst)
{
    const int count = ftgp_net_caller_floats(n_layers, width);
    const size_t stride = (size_t)ftgp_net_member_stride(ftgp_net_library_floats(n_layers, width));
    for (size_t m = 0; m < (size_t)n_members; ++m)
        for (int i = 0; i < count; ++i) dst[m * (size_t)count + (size_t)i] = img[m * stride + (size_t)ftgp_net_library_index(n_layers, width, i)];
}
