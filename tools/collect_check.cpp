// Host harness: the element operations of a collected decision's step 1 -- the mean, the noise, the clip and the guard -- with the
// SHIPPED functions (csrc/ftgp_net.h) in the written order of include/ftgp.h "Collected rollouts", as the act kernel's two lanes apply
// them, on the CPU; writes mean and action as raw binary, for tests/test_collect.py to compare bit for bit with the numpy model of the
// header's text (tests/collect_model.py).
// Build: c++ -O2 -ffp-contract=off -std=c++17 tools/collect_check.cpp -o /tmp/collect_check        (no HIP needed)
//        (the test also builds it with -fsanitize=address,undefined)
// Input:  int32 n; float scale[2], offset[2], std[2], lo[2], hi[2]; float y[n][2]; float noise[n][2].
// Output: float mean[n][2]; float action[n][2].
#include "../ft_grandprix_amd/csrc/ftgp_net.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: collect_check in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb"); if (!f) { perror("open"); return 2; }
    int32_t n = 0; float g[10];
    if (fread(&n, 4, 1, f) != 1 || fread(g, 4, 10, f) != 10 || n < 1 || n > (1 << 24)) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
    const float* scale = g; const float* offset = g + 2; const float* std_ = g + 4; const float* lo = g + 6; const float* hi = g + 8;
    std::vector<float> y((size_t)n * 2), noise((size_t)n * 2), mean((size_t)n * 2), action((size_t)n * 2);
    if (fread(y.data(), 4, y.size(), f) != y.size() || fread(noise.data(), 4, noise.size(), f) != noise.size()) { fprintf(stderr, "short input\n"); fclose(f); return 2; }
    fclose(f);
    for (int i = 0; i < n; ++i) {
        float a[2];
        for (int k = 0; k < 2; ++k) {
            const float m = ftgp_net_mean(y[2 * (size_t)i + k], scale[k], offset[k]);
            mean[2 * (size_t)i + k] = m;
            a[k] = ftgp_net_clip(ftgp_net_noisy(m, std_[k], noise[2 * (size_t)i + k]), lo[k], hi[k]);
        }
        const bool both = ftgp_net_finite(a[0]) && ftgp_net_finite(a[1]);
        for (int k = 0; k < 2; ++k) action[2 * (size_t)i + k] = ftgp_net_guarded(a[k], both);
    }
    FILE* o = fopen(argv[2], "wb"); if (!o) { perror("open"); return 2; }
    fwrite(mean.data(), 4, mean.size(), o);
    fwrite(action.data(), 4, action.size(), o);
    fclose(o);
    return 0;
}
