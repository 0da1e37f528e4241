// net_layout_check.cpp -- host harness of a network population's parameter layout (include/ftgp.h: ftgp_set_net_population): the
// conversion from the caller's layout to the library's member-strided one and back, with the shipped functions of csrc/ftgp_net.h --
// the ones ftgp_set_net, ftgp_set_net_population, the getters and ftgp_net_params_kernel call.
// Build: c++ -O2 -std=c++17 tools/net_layout_check.cpp -o /tmp/net_layout_check        (no HIP needed)
// Usage: net_layout_check in.bin out.bin
//   in.bin : int32 n_layers, width[FTGP_NET_MAX_LAYERS + 1] (width[0] = n_in, then the outputs per layer), n_members;
//            float32 params[n_members][count] in the caller's layout
//   out.bin: int32 count, library floats, member stride; float32 img[n_members][stride], from a buffer of zeros as the setter's is;
//            float32 back[n_members][count], img converted back; int32 index[count], ftgp_net_library_index of every parameter, then
//            the index of -1 and of count (both -1)
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../ft_grandprix_amd/csrc/ftgp_net.h"

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: net_layout_check in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t n_layers = 0, width[FTGP_NET_MAX_LAYERS + 1] = {}, n_members = 0;
    if (fread(&n_layers, 4, 1, f) != 1 || fread(width, 4, FTGP_NET_MAX_LAYERS + 1, f) != FTGP_NET_MAX_LAYERS + 1 || fread(&n_members, 4, 1, f) != 1) return 1;
    if (n_layers < 1 || n_layers > FTGP_NET_MAX_LAYERS || n_members < 1) return 1;
    const int32_t count = ftgp_net_caller_floats(n_layers, width), lib = ftgp_net_library_floats(n_layers, width), stride = ftgp_net_member_stride(lib);
    std::vector<float> src((size_t)n_members * count), img((size_t)n_members * stride, 0.0f), back((size_t)n_members * count, -1.0f);
    if (fread(src.data(), 4, src.size(), f) != src.size()) return 1;
    fclose(f);
    ftgp_net_population_to_library(n_layers, width, n_members, src.data(), img.data());
    ftgp_net_population_from_library(n_layers, width, n_members, img.data(), back.data());
    std::vector<int32_t> index((size_t)count + 2);
    for (int i = 0; i < count; ++i) index[(size_t)i] = ftgp_net_library_index(n_layers, width, i);
    index[(size_t)count] = ftgp_net_library_index(n_layers, width, -1);
    index[(size_t)count + 1] = ftgp_net_library_index(n_layers, width, count);
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    const int32_t head[3] = { count, lib, stride };
    fwrite(head, 4, 3, o);
    fwrite(img.data(), 4, img.size(), o);
    fwrite(back.data(), 4, back.size(), o);
    fwrite(index.data(), 4, index.size(), o);
    fclose(o);
    return 0;
}
