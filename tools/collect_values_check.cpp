// Host harness: the advantage scan of include/ftgp.h "Collected rollouts with values" and the value element, with the SHIPPED functions
// (csrc/ftgp_net.h: ftgp_gae_step, ftgp_gae_return, ftgp_net_value) in the written order, as ftgp_gae_kernel applies them -- one row after
// the other, t descending -- on the CPU; writes advantage, ret and the value elements as raw binary, for tests/test_collect_values.py to
// compare bit for bit with the numpy model of the header's text (tests/collect_values_model.py).
// Build: c++ -O2 -ffp-contract=off -std=c++17 tools/collect_values_check.cpp -o /tmp/collect_values_check        (no HIP needed)
//        (the test also builds it with -fsanitize=address,undefined)
// Input:  int32 T, n_envs, n_ext, n_y; float gamma, lam, scale, offset; float reward[T][n_envs][n_ext], value[..], next_value[..];
//         uint8 terminated[T][n_envs], truncated[T][n_envs]; float y[n_y].
// Output: float advantage[T][n_envs][n_ext]; float ret[T][n_envs][n_ext]; float v[n_y] = the value element of y.
#include "../ft_grandprix_amd/csrc/ftgp_net.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: collect_values_check in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb"); if (!f) { perror("open"); return 2; }
    int32_t h[4] = { 0, 0, 0, 0 }; float g[4];
    if (fread(h, 4, 4, f) != 4 || fread(g, 4, 4, f) != 4) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
    const int T = h[0], n_envs = h[1], n_ext = h[2], n_y = h[3];
    if (T < 1 || n_envs < 1 || n_ext < 1 || n_y < 0 || T > (1 << 16) || n_envs > (1 << 16) || n_ext > 8 || n_y > (1 << 24)) { fprintf(stderr, "bad sizes\n"); fclose(f); return 2; }
    const size_t rows = (size_t)n_envs * (size_t)n_ext, n = (size_t)T * rows, ne = (size_t)T * (size_t)n_envs;
    std::vector<float> reward(n), value(n), next_value(n), advantage(n), ret(n), y((size_t)n_y), v((size_t)n_y);
    std::vector<uint8_t> terminated(ne), truncated(ne);
    if (fread(reward.data(), 4, n, f) != n || fread(value.data(), 4, n, f) != n || fread(next_value.data(), 4, n, f) != n ||
        fread(terminated.data(), 1, ne, f) != ne || fread(truncated.data(), 1, ne, f) != ne || (!y.empty() && fread(y.data(), 4, y.size(), f) != y.size())) {
        fprintf(stderr, "short input\n"); fclose(f); return 2;
    }
    fclose(f);
    const float gamma = g[0], lam = g[1];
    const float gl = gamma * lam;                                 // rounded once
    for (size_t row = 0; row < rows; ++row) {
        const size_t env = row / (size_t)n_ext;
        float a = 0.0f;
        for (int t = T - 1; t >= 0; --t) {
            const size_t at = (size_t)t * rows + row, ae = (size_t)t * (size_t)n_envs + env;
            a = ftgp_gae_step(gamma, gl, reward[at], value[at], next_value[at], terminated[ae] != 0, truncated[ae] != 0, t == T - 1, a);
            advantage[at] = a;
            ret[at] = ftgp_gae_return(a, value[at]);
        }
    }
    for (size_t i = 0; i < y.size(); ++i) v[i] = ftgp_net_value(y[i], g[2], g[3]);
    FILE* o = fopen(argv[2], "wb"); if (!o) { perror("open"); return 2; }
    fwrite(advantage.data(), 4, n, o);
    fwrite(ret.data(), 4, n, o);
    if (!v.empty()) fwrite(v.data(), 4, v.size(), o);
    fclose(o);
    return 0;
}
