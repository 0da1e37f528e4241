// Host harness: runs the SHIPPED start-table builder and spawn draw (ftgp_spawn.h) on the CPU and writes what they give as raw binary,
// for tests/test_spawn_rule.py to compare bit for bit with the numpy model of include/ftgp.h's text (tests/spawn_model.py).
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -std=c++17 -x hip tools/spawn_check.cpp -o /tmp/spawn_check
// Input:  int32 W, H, wpr, 0; double px_size_x, px_size_y, origin_x, origin_y; double path[100][2]; uint32 bits[H * wpr].
// Output: double table[100][6] (x, y, qw, qz, clear_left, clear_right); int32 n_start, start[100] (unused entries -1);
//         double pose[episodes][n_envs][cars][4] (x, y, qw, qz); int32 draw[episodes][n_envs][cars][4] (p, slot, offset, 0).
// Reals on the command line may be written as hexadecimal floats (strtod reads them exactly).
#include "../ft_grandprix_amd/csrc/ftgp_spawn.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 14) {
        fprintf(stderr, "usage: spawn_check track.raw out.bin seed env_base n_envs cars episodes first_point n_points shuffle margin lateral_frac yaw_tan\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb"); if (!f) { perror("open"); return 2; }
    int32_t hdr[4]; double geo[4];
    std::vector<double> path(2 * FTGP_PATH_POINTS);
    if (fread(hdr, 4, 4, f) != 4 || fread(geo, 8, 4, f) != 4 || fread(path.data(), 8, path.size(), f) != path.size()) return 2;
    if (hdr[0] < 1 || hdr[1] < 1 || hdr[2] != (hdr[0] + 31) / 32) { fprintf(stderr, "bad image header\n"); return 2; }
    std::vector<uint32_t> bits((size_t)hdr[1] * hdr[2]);
    if (fread(bits.data(), 4, bits.size(), f) != bits.size()) return 2;
    fclose(f);
    const uint64_t seed = strtoull(argv[3], nullptr, 0);
    const int env_base = atoi(argv[4]), n_envs = atoi(argv[5]), cars = atoi(argv[6]), episodes = atoi(argv[7]);
    FtgpSpawnRule r{};
    r.first_point = atoi(argv[8]); r.n_points = atoi(argv[9]); r.shuffle_grid = atoi(argv[10]);
    r.margin = strtod(argv[11], nullptr); r.lateral_frac = strtod(argv[12], nullptr); r.yaw_tan = strtod(argv[13], nullptr);
    if (n_envs < 1 || cars < 1 || cars > 8 || episodes < 1 || r.first_point < 0 || r.first_point >= FTGP_PATH_POINTS || r.n_points < 1 || r.n_points > FTGP_PATH_POINTS) {
        fprintf(stderr, "bad arguments\n"); return 2;
    }
    FtgpTrack t{};
    t.width = hdr[0]; t.height = hdr[1]; t.words_per_row = hdr[2]; t.bits = bits.data();
    t.px_size_x = geo[0]; t.px_size_y = geo[1]; t.origin_x = geo[2]; t.origin_y = geo[3]; t.path = path.data();
    std::vector<double> spawn(4 * FTGP_PATH_POINTS), clear(2 * FTGP_PATH_POINTS), table(6 * FTGP_PATH_POINTS);
    ftgp_spawn_table(t, spawn.data());
    ftgp_start_table(t, spawn.data(), clear.data());
    for (int p = 0; p < FTGP_PATH_POINTS; ++p) {
        for (int q = 0; q < 4; ++q) table[6 * p + q] = spawn[4 * p + q];
        table[6 * p + 4] = clear[2 * p]; table[6 * p + 5] = clear[2 * p + 1];
    }
    std::vector<int32_t> start(FTGP_PATH_POINTS, -1);
    const int32_t n_start = ftgp_start_list(r, clear.data(), start.data());
    FILE* o = fopen(argv[2], "wb"); if (!o) { perror("open"); return 2; }
    fwrite(table.data(), 8, table.size(), o);
    fwrite(&n_start, 4, 1, o);
    fwrite(start.data(), 4, start.size(), o);
    if (n_start == 0) { fclose(o); printf("no start point\n"); return 3; }
    const size_t n = (size_t)episodes * n_envs * cars;
    std::vector<double> pose(4 * n); std::vector<int32_t> draw(4 * n);
    size_t i = 0;
    for (int k = 0; k < episodes; ++k)
        for (int e = 0; e < n_envs; ++e)
            for (int a = 0; a < cars; ++a, ++i) {
                FtgpSpawnPose s;
                ftgp_spawn_draw(seed, (uint64_t)(env_base + e), (uint64_t)k, cars, a, start.data(), n_start, clear.data(), spawn.data(),
                                r.margin, r.lateral_frac, r.yaw_tan, r.shuffle_grid, s);
                pose[4 * i] = s.x; pose[4 * i + 1] = s.y; pose[4 * i + 2] = s.qw; pose[4 * i + 3] = s.qz;
                draw[4 * i] = s.p; draw[4 * i + 1] = s.slot; draw[4 * i + 2] = s.offset; draw[4 * i + 3] = 0;
            }
    fwrite(pose.data(), 8, pose.size(), o);
    fwrite(draw.data(), 4, draw.size(), o);
    fclose(o);
    printf("%d start points, %zu draws\n", (int)n_start, n);
    return 0;
}
