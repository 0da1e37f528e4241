// ftgp_train.h -- training on the device (include/ftgp.h "Training on the device": ftgp_train_grad_device, ftgp_train_adam_device): the
// gradient of the clipped-PPO objective over rows of a collected rollout, and an Adam step on a slot's policy and value net in place.
// Included behind the last kernel of ftgp_kernels.hip, so that the code object keeps every other kernel where it was.
// (Like ftgp_net.h this file is not among the hashed kernel sources: after a change here alone, rebuild with build(force=True).)
//
// ftgp_train_grad_kernel<R>: workgroup g of G = min(tiles, FTGP_TRAIN_MAX_WG) takes the tiles g, g + G, .. of R batch rows (R = 32, or 16
// where 32 rows of the largest shapes would not fit 64 KiB of LDS).  A tile's rows live in LDS, row_floats apart: the input x, the stored
// outputs of every layer of the net in hand, and two delta buffers of ld_max floats.  The policy first, then the value net, each: forward
// (wave w the rows w*R/4 .., lane j the neurons j and j + 64: the header's fmaf chain from the bias, k ascending, so new_mean and new_value
// are what ftgp_collect_device wrote), the output delta (one thread per row), then per layer from the last one the weight gradient
// dWt[k][j] = sum over the tile's rows r ascending of x[r][k] * dA[r][j] (k = n_in is the bias) and the input delta dX[r][k] = sum over j
// of dA[r][j] * Wt[k][j], times the activation's derivative from the stored output -- both on v_mfma_f32_32x32x2_f32, 32 x 32 tiles of
// the result dealt to the four waves (train_dw, train_dx); the forward stays a plain fmaf chain, which the specification allows.
// A workgroup adds its tiles, in the order it takes them, into ITS OWN partial sums part[g] (the library's layout, the padding zeros);
// ftgp_train_reduce_kernel adds the partial sums g = 0, 1, .. in that order and divides by S.  No floating-point atomics anywhere: the
// number and the order of the sums follow from the shapes alone.  The numerators of stats [1] .. [4] take the same path in binary64
// (part_wide) and are rounded once, after the division by S: their error does not grow with the batch.
#pragma once
#include "ftgp_net.h"

#define FTGP_TRAIN_MAX_WG 256
#define FTGP_TRAIN_THREADS 256
#define FTGP_TRAIN_ROWSTATS 6        // per row: w, w*s, w*(v - ret)^2/2, w*(logq - logp), w*[|rho - 1| > c], refused

struct TrainNet {                    // one of a slot's two nets as the train kernels read it
    int32_t n_layers, hidden_act, out_act, n_floats;
    int32_t width[FTGP_NET_MAX_LAYERS + 1], w_off[FTGP_NET_MAX_LAYERS], b_off[FTGP_NET_MAX_LAYERS];     // as NetDev
    int32_t x_off[FTGP_NET_MAX_LAYERS + 1];      // where the outputs of layer l - 1 sit in an LDS row (x_off[0] = 0: the input), multiples of 4
    float out_scale[2], out_offset[2];
    const float* params;             // the library's layout: what ftgp_set_net_device / ftgp_set_value_net_device write
    int32_t g_off, pad;              // this net's first float in the trainer's gradient and moments
};
struct TrainArgs {
    TrainNet net[2];                 // the policy, the value net
    int32_t n_rows, n_batch, first_row, n_tiles;
    int32_t row_floats, d_off[2], n_total;       // an LDS row; its two delta buffers; the floats of both gradients
    const int32_t* index;
    const float* inputs; const float* mean; const float* noise; const float* advantage; const float* ret; const float* weight;
    float std[2], clip, value_coef;
    float* new_mean; float* new_value;
    float* part;                     // [G][n_total] the workgroups' partial sums
    float* part_stats;               // [G][FTGP_TRAIN_STATS]
    double* part_wide;               // [G][4]: the binary64 sums of columns 1 .. 4
};

typedef float train_f32x16 __attribute__((ext_vector_type(16)));      // the accumulator of v_mfma_f32_32x32x2_f32

__device__ __forceinline__ float train_act_slope(int act, float o)      // the activation's derivative from its stored output
{
    return act == FTGP_ACT_TANH ? 1.0f - o * o : act == FTGP_ACT_RELU ? (o > 0.0f ? 1.0f : 0.0f) : 1.0f;
}

// one layer forward on RW rows of a wave: "Layers" of include/ftgp.h to the letter
template <int RW>
__device__ __forceinline__ void train_forward(const float* __restrict__ params, int w_off, int b_off, int n_in, int n_out, int act,
                                              const float* in, float* out, int S, int lane)
{
    const int ld = ftgp_net_ld(n_out);
    const bool two = ld > FTGP_WAVE;
    const float* __restrict__ W = params + w_off + lane;
    const float b0 = params[b_off + lane], b1 = two ? params[b_off + FTGP_WAVE + lane] : 0.0f;
    float a0[RW], a1[RW];
    #pragma unroll
    for (int r = 0; r < RW; ++r) { a0[r] = b0; a1[r] = b1; }
    int k = 0;
    // (eight rows of weights in flight before the first of them is used: a workgroup has one wave per SIMD and nothing else hides the loads;
    // the chain of every neuron stays k ascending)
    for (; k + 8 <= n_in; k += 8) {
        float w0[8], w1[8];
        #pragma unroll
        for (int u = 0; u < 8; ++u) { w0[u] = W[(size_t)(k + u) * ld]; w1[u] = two ? W[(size_t)(k + u) * ld + FTGP_WAVE] : 0.0f; }
        #pragma unroll
        for (int u = 0; u < 8; ++u) {
            #pragma unroll
            for (int r = 0; r < RW; ++r) {
                const float x = in[r * S + k + u];
                a0[r] = fmaf(w0[u], x, a0[r]);
                if (two) a1[r] = fmaf(w1[u], x, a1[r]);
            }
        }
    }
    for (; k < n_in; ++k) {
        const float w0 = W[(size_t)k * ld], w1 = two ? W[(size_t)k * ld + FTGP_WAVE] : 0.0f;
        #pragma unroll
        for (int r = 0; r < RW; ++r) {
            const float x = in[r * S + k];
            a0[r] = fmaf(w0, x, a0[r]);
            if (two) a1[r] = fmaf(w1, x, a1[r]);
        }
    }
    const int n4 = (n_out + 3) & ~3;         // (the row's slot is padded to 4 floats with zeros: the float4 reads of the input delta)
    #pragma unroll
    for (int r = 0; r < RW; ++r) {
        if (lane < n4) out[r * S + lane] = lane < n_out ? ftgp_net_act(act, a0[r]) : 0.0f;
        if (two && lane + FTGP_WAVE < n4) out[r * S + FTGP_WAVE + lane] = lane + FTGP_WAVE < n_out ? ftgp_net_act(act, a1[r]) : 0.0f;
    }
}

// the weight and bias gradient of one layer over the R rows of a tile, into the workgroup's partial sums
template <int R>
__device__ __forceinline__ void train_dw(float* __restrict__ P, bool first, int w_off, int b_off, int n_in, int n_out,
                                         const float* in, const float* dA, int S, int lane, int wave)
{
    // dWt = X^T dA on v_mfma_f32_32x32x2_f32: a 32 x 32 tile of (k, j) per wave at a time, K = the tile's rows r, two per instruction
    // (A: lane l holds x[r = 2s + l / 32][k0 + l % 32], B: dA[r][j0 + l % 32]; C: column j0 + l % 32, row k0 + (q & 3) + 8 (q >> 2) +
    // 4 (l / 32) in register q).  Row k = n_in is the bias (x = 1).  Rows past it are computed from whatever lies behind the layer's
    // inputs in the LDS row -- inside the row: two delta buffers follow -- and dropped: a row of C depends on its own row of A alone.
    const int ld = ftgp_net_ld(n_out);
    const int kt = (n_in + 1 + 31) >> 5, jt = ld >> 5;
    const int c = lane & 31, h = lane >> 5;
    for (int t = wave; t < kt * jt; t += FTGP_TRAIN_THREADS / FTGP_WAVE) {
        const int k0 = (t / jt) << 5, j0 = (t % jt) << 5;
        const int k = k0 + c;
        train_f32x16 acc;
        #pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        #pragma unroll
        for (int s = 0; s < R / 2; ++s) {
            const int r = 2 * s + h;
            const float a = k == n_in ? 1.0f : in[r * S + k];
            const float b = dA[r * S + j0 + c];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        #pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int kk = k0 + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (kk <= n_in) {
                float* o = P + (kk < n_in ? w_off + kk * ld : b_off) + j0 + c;
                if (first) o[0] = acc[q]; else o[0] += acc[q];
            }
        }
    }
}

// The delta of the layer below over the R rows of a tile: dX = dA W on v_mfma_f32_32x32x2_f32, a 32 x 32 tile of (r, k) per wave at a
// time, K = the layer's outputs j.  The order of j inside the sum is free, so eight of them go through four instructions with lane
// half h holding j0 + 4h .. j0 + 4h + 3 of both operands -- one 16-byte load of the weights' row k and one of the delta's row r per
// four instructions (A: dA[r = l % 32][j], B: Wt[k0 + l % 32][j]; C: column k, row r = (q & 3) + 8 (q >> 2) + 4 (l / 32)).  The
// weights' padding and the delta's are zeros up to ld, so j runs to n_out rounded up to 8.  With R = 16 the rows 16 .. 31 repeat row
// 15 and are dropped; a column past n_in reads the weights' last row and stores 0: the delta is zeros up to ld(n_in).
template <int R>
__device__ __forceinline__ void train_dx(const float* __restrict__ params, int w_off, int n_in, int n_out, int act_below,
                                         const float* h, const float* dA, float* dnext, int S, int lane, int wave)
{
    const int ld = ftgp_net_ld(n_out), ldin = ftgp_net_ld(n_in);
    const int n8 = (n_out + 7) & ~7;
    const int c = lane & 31, hh = lane >> 5;
    const float* dr = dA + (c < R ? c : R - 1) * S + 4 * hh;
    for (int t = wave; t < (ldin >> 5); t += FTGP_TRAIN_THREADS / FTGP_WAVE) {
        const int k = (t << 5) + c;
        const float* __restrict__ Wk = params + w_off + (size_t)(k < n_in ? k : n_in - 1) * ld + 4 * hh;
        train_f32x16 acc;
        #pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        #pragma unroll 2
        for (int j0 = 0; j0 < n8; j0 += 8) {
            const float4 w = *reinterpret_cast<const float4*>(Wk + j0);
            const float4 d = *reinterpret_cast<const float4*>(dr + j0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d.x, w.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d.y, w.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d.z, w.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d.w, w.w, acc, 0, 0, 0);
        }
        #pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = (q & 3) + 8 * (q >> 2) + 4 * hh;
            if (r < R) dnext[r * S + k] = k < n_in ? acc[q] * train_act_slope(act_below, h[r * S + k]) : 0.0f;
        }
    }
}

template <int R>
__global__ void __launch_bounds__(FTGP_TRAIN_THREADS) ftgp_train_grad_kernel(TrainArgs T)
{
    extern __shared__ __attribute__((aligned(16))) float train_rows[];       // [R][row_floats]
    __shared__ int rowid[R];                                                 // the row of the caller's buffers, -1 = none
    __shared__ float rowstat[R][FTGP_TRAIN_ROWSTATS];
    constexpr int RW = R / (FTGP_TRAIN_THREADS / FTGP_WAVE);
    const int tid = (int)threadIdx.x, lane = tid & (FTGP_WAVE - 1), wave = tid >> 6;
    const int S = T.row_floats;
    float* __restrict__ P = T.part + (size_t)blockIdx.x * (size_t)T.n_total;
    // thread t < FTGP_TRAIN_ROWSTATS: the workgroup's sum of column t.  Columns 0 (w: S divides the gradient) and 5 (the rows refused) are
    // binary32 sums; columns 1 .. 4, the numerators of stats [1] .. [4], are carried in binary64, so that what a stat loses does not grow
    // with the number of rows
    float stat = 0.0f;
    double wide = 0.0;
    const bool is_wide = tid >= 1 && tid <= 4;
    bool first = true;
    for (int tile = (int)blockIdx.x; tile < T.n_tiles; tile += (int)gridDim.x, first = false) {
        // ---- the tile's rows: a row number outside [0, n_rows) is counted and never dereferenced
        if (tid < R) {
            const int64_t i = (int64_t)tile * R + tid;
            int row = -1;
            float refused = 0.0f;
            if (i < (int64_t)T.n_batch) {
                const int64_t want = T.index ? (int64_t)T.index[i] : (int64_t)T.first_row + i;
                if (want >= 0 && want < (int64_t)T.n_rows) row = (int)want; else refused = 1.0f;
            }
            rowid[tid] = row;
            #pragma unroll
            for (int q = 0; q < FTGP_TRAIN_ROWSTATS - 1; ++q) rowstat[tid][q] = 0.0f;
            rowstat[tid][FTGP_TRAIN_ROWSTATS - 1] = refused;
        }
        __syncthreads();
        {
            const int n_in = T.net[0].width[0], n4 = (n_in + 3) & ~3;
            for (int at = tid; at < R * n4; at += FTGP_TRAIN_THREADS) {
                const int r = at / n4, k = at - r * n4, row = rowid[r];
                train_rows[r * S + k] = (row >= 0 && k < n_in) ? T.inputs[(size_t)row * (size_t)n_in + (size_t)k] : 0.0f;
            }
        }
        __syncthreads();
        #pragma unroll 1
        for (int which = 0; which < 2; ++which) {
            const TrainNet& N = T.net[which];
            const int L = N.n_layers;
            float* mine = train_rows + wave * RW * S;            // this wave's rows
            #pragma unroll 1
            for (int l = 0; l < L; ++l) {
                train_forward<RW>(N.params, N.w_off[l], N.b_off[l], N.width[l], N.width[l + 1], l + 1 < L ? N.hidden_act : N.out_act,
                                  mine + N.x_off[l], mine + N.x_off[l + 1], S, lane);
                __syncthreads();
            }
            // ---- the output delta, one thread per row; the delta buffer is zeros up to the last layer's ld = 64
            int cur = 0;
            if (tid < R) {
                const int row = rowid[tid];
                const int64_t i = (int64_t)tile * R + tid;
                const float* y = train_rows + tid * S + N.x_off[L];
                float* d = train_rows + tid * S + T.d_off[cur];
                float dk[2] = { 0.0f, 0.0f };
                if (which == 0) {
                    const float m0 = ftgp_net_mean(y[0], N.out_scale[0], N.out_offset[0]), m1 = ftgp_net_mean(y[1], N.out_scale[1], N.out_offset[1]);
                    if (row >= 0) {
                        const float w = T.weight ? T.weight[row] : 1.0f, A = T.advantage[row];
                        const float n0 = T.noise ? T.noise[2 * (size_t)row] : 0.0f, n1 = T.noise ? T.noise[2 * (size_t)row + 1] : 0.0f;
                        // z = (p - m) / std with p = std * noise + mean, written so that m == mean gives z == noise and a ratio of exactly 1
                        const float z0 = n0 + (T.mean[2 * (size_t)row] - m0) / T.std[0], z1 = n1 + (T.mean[2 * (size_t)row + 1] - m1) / T.std[1];
                        const float logp = -0.5f * (z0 * z0 + z1 * z1), logq = -0.5f * (n0 * n0 + n1 * n1);
                        const float rho = expf(logp - logq);
                        const float lo = 1.0f - T.clip, hi = 1.0f + T.clip;
                        const float cl = rho < lo ? lo : (rho > hi ? hi : rho);
                        const float s1 = rho * A, s2 = cl * A, s = s1 < s2 ? s1 : s2;
                        // (0 where the clip binds; a NaN advantage or ratio binds nothing and reaches the gradient: the non-finite flag's business)
                        const bool clipped = (A >= 0.0f && rho > hi) || (A < 0.0f && rho < lo);
                        const float up = clipped ? 0.0f : -(w * A * rho);            // S * dL/dlogp = S * rho * dL/drho
                        dk[0] = up * (z0 / T.std[0]) * N.out_scale[0] * train_act_slope(N.out_act, y[0]);
                        dk[1] = up * (z1 / T.std[1]) * N.out_scale[1] * train_act_slope(N.out_act, y[1]);
                        rowstat[tid][0] = w; rowstat[tid][1] = -(w * s); rowstat[tid][3] = w * (logq - logp);
                        rowstat[tid][4] = fabsf(rho - 1.0f) > T.clip ? w : 0.0f;
                    }
                    if (T.new_mean && i < (int64_t)T.n_batch) { T.new_mean[2 * i] = row >= 0 ? m0 : 0.0f; T.new_mean[2 * i + 1] = row >= 0 ? m1 : 0.0f; }
                } else {
                    const float v = ftgp_net_value(y[0], N.out_scale[0], N.out_offset[0]);
                    if (row >= 0) {
                        const float w = T.weight ? T.weight[row] : 1.0f, e = v - T.ret[row];
                        dk[0] = T.value_coef * w * e * N.out_scale[0] * train_act_slope(N.out_act, y[0]);
                        rowstat[tid][2] = w * (0.5f * (e * e));
                    }
                    if (T.new_value && i < (int64_t)T.n_batch) T.new_value[i] = row >= 0 ? v : 0.0f;
                }
                d[0] = dk[0]; d[1] = which == 0 ? dk[1] : 0.0f;
                for (int j = 2; j < FTGP_WAVE; ++j) d[j] = 0.0f;
            }
            __syncthreads();
            // ---- backward, from the last layer
            #pragma unroll 1
            for (int l = L - 1; l >= 0; --l) {
                train_dw<R>(P + N.g_off, first, N.w_off[l], N.b_off[l], N.width[l], N.width[l + 1],
                            train_rows + N.x_off[l], train_rows + T.d_off[cur], S, lane, wave);
                if (l > 0)
                    train_dx<R>(N.params, N.w_off[l], N.width[l], N.width[l + 1], N.hidden_act,
                                train_rows + N.x_off[l], train_rows + T.d_off[cur], train_rows + T.d_off[cur ^ 1], S, lane, wave);
                __syncthreads();
                cur ^= 1;
            }
        }
        if (tid < FTGP_TRAIN_ROWSTATS) {
            if (is_wide) {
                double s = 0.0;
                for (int r = 0; r < R; ++r) s += (double)rowstat[r][tid];
                wide += s;
            } else {
                float s = 0.0f;
                for (int r = 0; r < R; ++r) s += rowstat[r][tid];
                stat += s;
            }
        }
        __syncthreads();
    }
    if (tid < FTGP_TRAIN_ROWSTATS) {
        float* mine = T.part_stats + (size_t)blockIdx.x * FTGP_TRAIN_STATS;
        if (is_wide) {
            mine[tid] = (float)wide;                                       // (not read: the reduce takes the binary64 sum)
            T.part_wide[(size_t)blockIdx.x * 4 + (tid - 1)] = wide;
        } else {
            mine[tid == FTGP_TRAIN_ROWSTATS - 1 ? 6 : tid] = stat;         // stats[6]: the rows refused
        }
        if (tid == 0) { mine[5] = 0.0f; mine[7] = 0.0f; }
    }
}
template __global__ void ftgp_train_grad_kernel<32>(TrainArgs);
template __global__ void ftgp_train_grad_kernel<16>(TrainArgs);

// The partial sums of G workgroups, g ascending, into the gradient, divided by S; the stats; the non-finite flag.
// sync[0]: 1 if an element of the gradient is not finite, sync[1]: the ticket of the workgroups that are done (both zeroed before the launch;
// integer atomics: their order does not reach a result).  The last workgroup writes the stats.
struct TrainReduceArgs {
    const float* part; const float* part_stats; int32_t G, n_total;
    float* grad; int32_t* sync; float* stats; float* stats_out;       // stats: the trainer's own; stats_out: the caller's, or null
    const double* part_wide;
};
__device__ __forceinline__ float train_sum_stat(const TrainReduceArgs& A, int q)
{
    float s = 0.0f;
    for (int g = 0; g < A.G; ++g) s += A.part_stats[(size_t)g * FTGP_TRAIN_STATS + q];
    return s;
}
// columns 1 .. 4: the workgroups' binary64 sums, g ascending, in binary64
__device__ __forceinline__ double train_sum_stat_wide(const TrainReduceArgs& A, int q)
{
    double s = 0.0;
    for (int g = 0; g < A.G; ++g) s += A.part_wide[(size_t)g * 4 + (q - 1)];
    return s;
}
__global__ void __launch_bounds__(256) ftgp_train_reduce_kernel(TrainReduceArgs A)
{
    __shared__ float S_all;
    __shared__ int last;
    if (threadIdx.x == 0) S_all = train_sum_stat(A, 0);
    __syncthreads();
    const float S = S_all;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    int bad = 0;
    if (i < A.n_total) {
        // two levels, both fixed by G alone: four running sums over g = q, q + 4, .. (four loads in flight), then (s0 + s1) + (s2 + s3)
        float s4[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        int g = 0;
        for (; g + 4 <= A.G; g += 4) {
            #pragma unroll
            for (int q = 0; q < 4; ++q) s4[q] += A.part[(size_t)(g + q) * (size_t)A.n_total + (size_t)i];
        }
        #pragma unroll
        for (int q = 0; q < 3; ++q) if (g + q < A.G) s4[q] += A.part[(size_t)(g + q) * (size_t)A.n_total + (size_t)i];
        const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        const float v = S > 0.0f ? s / S : 0.0f;
        A.grad[i] = v;
        bad = !ftgp_net_finite(v);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        if (bad) atomicOr(A.sync, 1);
        __threadfence();
        last = atomicAdd(A.sync + 1, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x < FTGP_TRAIN_STATS) {
        __threadfence();
        const int q = (int)threadIdx.x;
        float v = 0.0f;
        if (q == 0) v = S > 0.0f ? S : 0.0f;
        else if (q >= 1 && q <= 4) v = S > 0.0f ? (float)(train_sum_stat_wide(A, q) / (double)S) : 0.0f;     // one rounding
        else if (q == 5) v = atomicOr(A.sync, 0) ? 1.0f : 0.0f;
        else if (q == 6) v = train_sum_stat(A, 6);
        A.stats[q] = v;
        if (A.stats_out) A.stats_out[q] = v;
    }
}

// Adam over both nets in place (ftgp_adam_step of ftgp_net.h); nothing moves while the gradient's non-finite flag is set.  The padding
// of the library's layout has g = m = v = 0 and keeps its zeros: p - a * (0 / eps) = p.
struct TrainAdamArgs {
    float* p[2]; int32_t n[2];               // the policy's and the value net's parameters, n_floats each
    const float* grad; float* m; float* v; const int32_t* sync;
    float b1, b2, omb1, omb2, a, r, eps;
};
__global__ void __launch_bounds__(256) ftgp_train_adam_kernel(TrainAdamArgs A)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= A.n[0] + A.n[1] || A.sync[0] != 0) return;
    float* p = i < A.n[0] ? A.p[0] + i : A.p[1] + (i - A.n[0]);
    ftgp_adam_step(p, A.m + i, A.v + i, A.grad[i], A.b1, A.b2, A.omb1, A.omb2, A.a, A.r, A.eps);
}
