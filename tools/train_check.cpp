// Host harness: Adam's element step of include/ftgp.h "Training on the device" with the SHIPPED functions (csrc/ftgp_net.h:
// ftgp_adam_scalars, ftgp_adam_step) as ftgp_train_adam_kernel applies them -- one parameter after the other -- on the CPU; writes the six
// scalars and the new p, m and v as raw binary, for tests/test_train.py to compare bit for bit with the numpy model of the header's text
// (tests/train_model.py).
// Build: c++ -O2 -ffp-contract=off -std=c++17 tools/train_check.cpp -o /tmp/train_check        (no HIP needed)
//        (the test also builds it with -fsanitize=address,undefined)
// Input:  int32 n; int64 t; float beta1, beta2, eps, lr; float p[n], m[n], v[n], g[n].
// Output: float scalars[6] (b1, b2, 1 - b1, 1 - b2, a, r); float p[n], m[n], v[n] after the step.
#include "../ft_grandprix_amd/csrc/ftgp_net.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: train_check in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb"); if (!f) { perror("open"); return 2; }
    int32_t n32 = 0; int64_t t = 0; float h[4];
    if (fread(&n32, 4, 1, f) != 1 || fread(&t, 8, 1, f) != 1 || fread(h, 4, 4, f) != 4) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
    if (n32 < 1 || n32 > (1 << 24) || t < 1) { fprintf(stderr, "bad sizes\n"); fclose(f); return 2; }
    const size_t n = (size_t)n32;
    std::vector<float> p(n), m(n), v(n), g(n);
    if (fread(p.data(), 4, n, f) != n || fread(m.data(), 4, n, f) != n || fread(v.data(), 4, n, f) != n || fread(g.data(), 4, n, f) != n) {
        fprintf(stderr, "short input\n"); fclose(f); return 2;
    }
    fclose(f);
    float s[6];
    ftgp_adam_scalars(h[0], h[1], h[3], t, s);
    for (size_t i = 0; i < n; ++i) ftgp_adam_step(&p[i], &m[i], &v[i], g[i], s[0], s[1], s[2], s[3], s[4], s[5], h[2]);
    FILE* o = fopen(argv[2], "wb"); if (!o) { perror("open"); return 2; }
    fwrite(s, 4, 6, o);
    fwrite(p.data(), 4, n, o);
    fwrite(m.data(), 4, n, o);
    fwrite(v.data(), 4, n, o);
    fclose(o);
    return 0;
}
