// Host harness: evaluates a whole network driver with the SHIPPED element operations (csrc/ftgp_net.h) in the written order of
// include/ftgp.h "Network drivers" on the CPU, prints the controls and writes them as raw binary, for tests/test_net_driver.py to
// compare bit for bit with the numpy model of the header's text (tests/net_model.py).
// Build: c++ -O2 -ffp-contract=off -std=c++17 tools/net_check.cpp -o /tmp/net_check        (no HIP needed)
// Input:  int32 n_rays, n_cars, pool, beam_first, n_beams, use_state, n_layers, width[4], hidden_act, out_act, n_params;
//         float max_range, out_scale[2], out_offset[2]; float params[n_params] (ftgp_set_net's layout);
//         float ranges[n_cars][n_rays]; double record[n_cars][7] = qw, qz, vx, vy, wz, u_speed, u_steer.
// Output: double ctrl[n_cars][2].
// Frame mode (net_check --frame in.bin out.bin; include/ftgp.h: ftgp_set_net_frame): the network's frame inputs with the shipped element
// operations of csrc/ftgp_frame.h, for tests/test_net_frame.py and tests/net_frame_model.py.  The input has, behind out_offset, int32
// frame[3] = enabled, n_ahead, stride; n_params counts the first layer with the true n_in; a record is double[9] = qw, qz, vx, vy, wz,
// u_speed, u_steer, x, y; behind the records double path[100][2].  It prints every car's full input vector and its controls, and the
// output is float inputs[n_cars][n_in], then double ctrl[n_cars][2].
// Rivals mode (net_check --rivals in.bin out.bin; include/ftgp.h: ftgp_set_net_rivals): the frame mode's file with, behind frame[3], int32
// rivals[3] = enabled, n_rivals, cars_per_env, and behind the path int32 absolute_completion[n_cars], int32 finished[n_cars], int64
// finish_step[n_cars]: the records of whole envs, n_cars / cars_per_env of them one after the other on the one path.  The rival entries
// come from csrc/ftgp_rival.h (rival_place per car, rival_row per row) behind the frame entries; a finished car reads (0, 0) before its
// network is looked at.  Printed and written as in frame mode.
#include "../ft_grandprix_amd/csrc/ftgp_net.h"
#include "../ft_grandprix_amd/csrc/ftgp_frame.h"
#include "../ft_grandprix_amd/csrc/ftgp_rival.h"
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    const bool rival_mode = argc == 4 && !strcmp(argv[1], "--rivals");
    const bool frame_mode = rival_mode || (argc == 4 && !strcmp(argv[1], "--frame"));
    if (argc != 3 && !frame_mode) { fprintf(stderr, "usage: net_check [--frame | --rivals] in.bin out.bin\n"); return 2; }
    if (frame_mode) { ++argv; }
    FILE* f = fopen(argv[1], "rb"); if (!f) { perror("open"); return 2; }
    int32_t h[14]; float g[5];
    if (fread(h, 4, 14, f) != 14 || fread(g, 4, 5, f) != 5) return 2;
    FtgpNetFrame fr{};
    if (frame_mode) {
        int32_t q[3];
        if (fread(q, 4, 3, f) != 3) return 2;
        fr.enabled = q[0]; fr.n_ahead = q[1]; fr.stride = q[2];
        if ((fr.enabled != 0 && fr.enabled != 1) || fr.n_ahead < 0 || fr.n_ahead > FTGP_MAX_LOOKAHEAD || fr.stride < 1 || fr.stride > 50) { fprintf(stderr, "bad frame\n"); return 2; }
    }
    FtgpNetRivals rv{};
    int cpe = 1;
    if (rival_mode) {
        int32_t q[3];
        if (fread(q, 4, 3, f) != 3) return 2;
        rv.enabled = q[0]; rv.n_rivals = q[1]; cpe = q[2];
        if ((rv.enabled != 0 && rv.enabled != 1) || rv.n_rivals < 0 || rv.n_rivals > FTGP_MAX_RIVALS || cpe < 1 || cpe > FTGP_MAX_RIVALS + 1) { fprintf(stderr, "bad rivals\n"); return 2; }
    }
    const int n_frame = ftgp_net_frame_inputs(&fr), n_rival = ftgp_net_rival_inputs(&rv), rec_w = frame_mode ? 9 : 7;
    const int n_rays = h[0], n_cars = h[1];
    if (n_cars < 1 || n_cars % cpe) { fprintf(stderr, "bad car count\n"); return 2; }
    FtgpNetDesc d{};
    d.pool = h[2]; d.beam_first = h[3]; d.n_beams = h[4]; d.use_state = h[5]; d.n_layers = h[6];
    for (int l = 0; l < FTGP_NET_MAX_LAYERS; ++l) d.width[l] = h[7 + l];
    d.hidden_act = h[11]; d.out_act = h[12];
    d.max_range = g[0]; d.out_scale[0] = g[1]; d.out_scale[1] = g[2]; d.out_offset[0] = g[3]; d.out_offset[1] = g[4];
    const int eighth = (int)(n_rays / 8.0);
    if (n_rays < 1 || n_cars < 1 || d.pool < 1 || n_rays % d.pool || d.n_beams < 1 || d.n_layers < 1 || d.n_layers > FTGP_NET_MAX_LAYERS ||
        d.beam_first * d.pool < eighth || (d.beam_first + d.n_beams) * d.pool > n_rays - eighth || ftgp_net_inputs(&d) + n_frame + n_rival > FTGP_NET_MAX_INPUTS ||
        (size_t)h[13] != ftgp_net_param_count(&d) + (size_t)d.width[0] * (size_t)(n_frame + n_rival)) { fprintf(stderr, "bad description\n"); return 2; }
    std::vector<float> params((size_t)h[13]), ranges((size_t)n_cars * n_rays);
    std::vector<double> rec((size_t)n_cars * rec_w), ctrl((size_t)n_cars * 2), path((size_t)2 * FTGP_PATH_POINTS);
    if (fread(params.data(), 4, params.size(), f) != params.size() || fread(ranges.data(), 4, ranges.size(), f) != ranges.size() ||
        fread(rec.data(), 8, rec.size(), f) != rec.size()) return 2;
    if (frame_mode && fread(path.data(), 8, path.size(), f) != path.size()) return 2;
    std::vector<int32_t> abs_completion((size_t)n_cars), finished((size_t)n_cars);
    std::vector<int64_t> finish_step((size_t)n_cars);
    if (rival_mode && (fread(abs_completion.data(), 4, abs_completion.size(), f) != abs_completion.size() || fread(finished.data(), 4, finished.size(), f) != finished.size() ||
                       fread(finish_step.data(), 8, finish_step.size(), f) != finish_step.size())) return 2;
    fclose(f);
    // every car's contribution to its env's rival rows
    std::vector<RivalCar> rcar((size_t)n_cars);
    std::vector<double> rg((size_t)n_cars);
    if (n_rival)
        for (int c = 0; c < n_cars; ++c) {
            const double* r = &rec[(size_t)c * rec_w];
            double s;
            rival_place(path.data(), r[7], r[8], abs_completion[c], s, rg[c]);
            rcar[c] = rival_car(r[7], r[8], r[0], r[1], r[2], r[3], s);
        }
    const int n_in0 = ftgp_net_inputs(&d) + n_frame + n_rival;
    std::vector<float> inputs((size_t)n_cars * n_in0);
    const float inv = 1.0f / d.max_range;
    for (int c = 0; c < n_cars; ++c) {
        float x[FTGP_NET_MAX_INPUTS], y[FTGP_NET_MAX_INPUTS];
        for (int b = 0; b < d.n_beams; ++b) x[b] = ftgp_net_beam(&ranges[(size_t)c * n_rays + (size_t)(d.beam_first + b) * d.pool], d.pool, d.max_range, inv);
        const double* r = &rec[(size_t)c * rec_w];
        if (d.use_state) for (int q = 0; q < FTGP_NET_STATE_INPUTS; ++q) x[d.n_beams + q] = ftgp_net_state(q, r[0], r[1], r[2], r[3], r[4], r[5], r[6]);
        if (n_frame) frame_row(path.data(), r[7], r[8], r[0], r[1], fr.n_ahead, fr.stride, x + ftgp_net_inputs(&d));      // the frame entries come behind the state
        if (n_rival) {                                                                                                      // the rival entries come last
            const int e0 = c - c % cpe;
            rival_row(&rcar[e0], &rg[e0], &finish_step[e0], &finished[e0], cpe, c - e0, rv.n_rivals, x + ftgp_net_inputs(&d) + n_frame);
        }
        int n_in = n_in0;
        for (int k = 0; k < n_in0; ++k) inputs[(size_t)c * n_in0 + k] = x[k];
        if (frame_mode) {
            printf("car %d: inputs", c);
            for (int k = 0; k < n_in0; ++k) printf(" %a", (double)x[k]);
            printf("\n");
        }
        const float* p = params.data();
        for (int l = 0; l < d.n_layers; ++l) {
            const int n_out = d.width[l], act = l + 1 < d.n_layers ? d.hidden_act : d.out_act;
            const float* W = p; const float* B = p + (size_t)n_out * n_in;
            for (int j = 0; j < n_out; ++j) {
                float acc = B[j];
                for (int k = 0; k < n_in; ++k) acc = fmaf(W[(size_t)j * n_in + k], x[k], acc);
                y[j] = ftgp_net_act(act, acc);
            }
            for (int j = 0; j < n_out; ++j) x[j] = y[j];
            p = B + n_out; n_in = n_out;
        }
        ftgp_net_controls(x[0], x[1], d.out_scale, d.out_offset, &ctrl[2 * c], &ctrl[2 * c + 1]);
        if (rival_mode && finished[c]) { ctrl[2 * c] = 0.0; ctrl[2 * c + 1] = 0.0; }
        printf("car %d: speed %a steer %a\n", c, ctrl[2 * c], ctrl[2 * c + 1]);
    }
    FILE* o = fopen(argv[2], "wb"); if (!o) { perror("open"); return 2; }
    if (frame_mode) fwrite(inputs.data(), 4, inputs.size(), o);
    fwrite(ctrl.data(), 8, ctrl.size(), o);
    fclose(o);
    return 0;
}
