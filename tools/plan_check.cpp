// Host harness: runs ftgp_create's plan (plan() with one track: the workgroup shape, the fan, the sweep's task order and task tables) on the CPU, without a
// device, over a matrix of configurations, and checks what the step kernel relies on.
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -std=c++17 -x hip tools/plan_check.cpp -o /tmp/plan_check -ldl
#include "../ft_grandprix_amd/csrc/ftgp_api.hip"
#include "plan_digest.h"

static long g_fail = 0;
static Fnv g_digest;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAIL %s: ", label); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "plan_window_check.h"

// the binary32 fan is point-symmetric to the bit: ray j + n/2 is the negated ray j (both components, sign bits included)
static bool point_symmetric(const std::vector<float>& ray, int R)
{
    if (R % 2) return false;
    for (int j = 0; j < R / 2; ++j)
        for (int k = 0; k < 2; ++k) {
            uint32_t a, b;
            const float x = ray[2 * (size_t)j + k], y = ray[2 * (size_t)(j + R / 2) + k];
            memcpy(&a, &x, 4); memcpy(&b, &y, 4);
            if (x != x || b != (a ^ 0x80000000u)) return false;
        }
    return true;
}

// one configuration; returns 1 when the plan rejected it
static int check(const FtgpConfig& cfg, const Switches& sw, const char* label, bool first_table_ok = false)
{
    Plan pl;
    const int rc = plan(cfg, &cfg.track, &cfg.n_envs, 1, 256, sw, pl);
    const DeviceParams& P = pl.tracks[0].P;
    const int R = cfg.n_rays, cpe = cfg.cars_per_env;
    if (rc != 0) {
        // only a shape that does not fit: one env of the configuration over the 160 KiB of LDS
        DeviceParams Q = P;
        const int one_env = lds_layout(Q, cpe, 16);
        char want[256];
        snprintf(want, sizeof want, "one env of %d car(s) with a %d-ray scan does not fit the 160 KiB LDS", cpe, R);
        CHECK(rc == FTGP_ERR_ARG && strcmp(ftgp_last_error(), want) == 0 && one_env > 160 * 1024, "rejected (%d: %s)", rc, ftgp_last_error());
        printf("%s: rejected (%d): %s\n", label, rc, ftgp_last_error());
        return 1;
    }
    // workgroup shape and LDS
    const int cpb = P.cars_per_block;
    CHECK(cpb >= cpe && cpb % cpe == 0 && cpb <= FTGP_MAX_CARS_PER_BLOCK, "cars_per_block %d (cars_per_env %d)", cpb, cpe);
    CHECK(P.lds_bytes <= 80 * 1024 || (cpb == cpe && P.lds_bytes <= 160 * 1024), "lds_bytes %d with %d cars per workgroup", P.lds_bytes, cpb);
    // direction sectors by car count
    const long cars = (long)cfg.n_envs * cpe;
    const int sectors = cars >= 8192 ? 8 : cars >= 2048 ? 16 : 64;
    CHECK(P.n_sectors == sectors && P.n_planes == sectors, "%d sectors / %d planes for %ld cars (want %d)", P.n_sectors, P.n_planes, cars, sectors);
    // opposite-group pairs exactly when the fan allows them
    const bool pairs_expected = R % 2 == 0 && point_symmetric(pl.ray, R) && !sw.no_pairs;
    // (a pair split at the tail leaves two single groups, the second starting at first + n/2: off the single groups' multiples of 64 unless n/2 is one)
    bool pairs = false;
    for (int k = 0; k < P.tasks_per_car; ++k) pairs = pairs || (P.group_order[k] >> 16) != 0 || (P.group_order[k] & 0xffff) % FTGP_WAVE != 0;
    // (n/2 a multiple of 64 and every pair split at the tail, e.g. 128 rays: the list cannot tell, nothing to check)
    if (pairs || !pairs_expected || (R / 2) % FTGP_WAVE != 0 || P.tasks_per_car > 4) CHECK(pairs == pairs_expected, "opposite pairs %d, expected %d", (int)pairs, (int)pairs_expected);
    // both task tables: each ray of each car slot drawn exactly once, decoded as ftgp_device.h documents task_tab -- except where a pair is split
    // at the tail (FTGP_PAIR_TAIL) and its half holds fewer than 64 rays: the first single group then runs on into the opposite half (rays
    // n/2 .. first + 63), which the second covers too (the same ray twice, the same result: what the plan does, counted here)
    const int ntasks = cpb * P.tasks_per_car, half = R / 2;
    std::vector<int> times(R, 1);
    if (pairs)
        for (int k = 0; k < P.tasks_per_car; ++k) {
            const int j0 = P.group_order[k] & 0xffff;
            if ((P.group_order[k] >> 16) == 0 && j0 < half && j0 + FTGP_WAVE > half) for (int j = half; j < std::min(j0 + FTGP_WAVE, R); ++j) ++times[j];
        }
    long twice = 0;
    for (int v : times) twice += v - 1;
    CHECK(pl.tasks.size() == 2 * 4 * (size_t)ntasks, "task table of %zu ints for %d tasks", pl.tasks.size(), ntasks);
    for (int table = 0; table < 2; ++table) {
        std::vector<int> drawn((size_t)cpb * R, 0);
        for (int g = 0; g < ntasks; ++g) {
            const int32_t* d = &pl.tasks[4 * ((size_t)table * ntasks + g)];
            const uint32_t x = (uint32_t)d[0];
            const int j0 = x & 0x3fff, kind = (x >> 14) & 3, c = (x >> 16) & 15;
            CHECK(c == g % cpb && (d[1] >> 16) == g / cpb && (d[1] & 0xffff) == c * (int)sizeof(LidarFrame), "draw %d: slot %d, rank %d", g, c, d[1] >> 16);
            CHECK(d[2] == c * P.ranges_stride * 4 && d[3] == 4 * (c * P.win_floats + (P.eighth & 3) - P.eighth), "draw %d: row offsets", g);
            // the second table: ray, kind and slot only (window classes 0, no ray-0 flag); the first flags the draw that holds ray 0
            if (table == 1) CHECK(x == ((uint32_t)pl.tasks[4 * (size_t)g] & 0xfffffu), "draw %d: the second table carries more than ray, kind and slot", g);
            else CHECK((int)((x >> 24) & 1) == (j0 == 0 ? 1 : 0) && (x >> 25) == 0, "draw %d: ray-0 flag", g);
            const int w0 = (x >> 20) & 3, w1 = (x >> 22) & 3;
            CHECK(kind != 3, "draw %d: kind 3", g);
            for (int lane = 0; lane < FTGP_WAVE; ++lane) {       // the lanes of the sweep's draw (lidar_groups)
                int j; bool mine;
                if (kind == 2) { j = j0 + (lane & 31) + (lane >= 32 ? half : 0); mine = (lane & 31) < half - j0; }
                else { j = j0 + lane; mine = j < (kind == 1 ? half : R); }
                if (!mine) continue;
                CHECK(j >= 0 && j < R, "draw %d: ray %d", g, j);
                if (j < 0 || j >= R) continue;
                ++drawn[(size_t)c * R + j];
                if (kind == 1) ++drawn[(size_t)c * R + j + half];
                // window classes against the drivers' scan window [eighth, R - eighth): 0 = no ray of the group in it, 1 = every ray, 2 = test per ray
                auto in_window = [&](int r) { return r >= P.eighth && r < R - P.eighth; };
                if (table == 1) continue;
                CHECK(w0 == 2 || w0 == (in_window(j) ? 1 : 0), "draw %d: window class %d of ray %d", g, w0, j);
                if (kind == 1) CHECK(w1 == 2 || w1 == (in_window(j + half) ? 1 : 0), "draw %d: window class %d of ray %d", g, w1, j + half);
                else CHECK(w1 == 0, "draw %d: second window class %d without a second group", g, w1);
            }
        }
        long bad = 0;
        for (size_t i = 0; i < drawn.size(); ++i) bad += drawn[i] != times[i % R];
        CHECK(bad == 0, "table %d: %ld (car slot, ray) not drawn exactly once (or twice where counted above)", table, bad);
    }
    check_window_table(pl, times, label, sw.scan_every_step, first_table_ok);
    Images im;
    layout_images(pl, made_up_addrs(pl), im);
    CHECK(im.params.size() >= FTGP_PARAMS_BYTES + sizeof(int32_t) * (pl.tasks.size() + pl.tasks_win.size()) &&
          memcmp(im.params.data() + FTGP_PARAMS_BYTES, pl.tasks.data(), sizeof(int32_t) * pl.tasks.size()) == 0 &&
          memcmp(im.params.data() + FTGP_PARAMS_BYTES + sizeof(int32_t) * pl.tasks.size(), pl.tasks_win.data(), sizeof(int32_t) * pl.tasks_win.size()) == 0,
          "the parameter image: the two task tables, then the window-only table");
    digest_plan(g_digest, pl, im);
    printf("%s: ok, %d x %d waves, %d B of LDS, %d sectors, %d tasks per car%s (%d window-only), %ld rays drawn twice\n", label, cpb, P.waves_per_block, P.lds_bytes, P.n_sectors,
           P.tasks_per_car, pairs ? " (pairs)" : "", P.win_tasks_per_car, twice);
    return 0;
}

int main()
{
    // a walled 160 x 120 image and an elliptical centre-line
    const int W = 160, H = 120, wpr = (W + 31) / 32;
    std::vector<uint32_t> bits((size_t)H * wpr, 0u);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) bits[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31);
    std::vector<double> path(2 * FTGP_PATH_POINTS);
    for (int p = 0; p < FTGP_PATH_POINTS; ++p) {
        path[2 * p] = 4.0 + 2.5 * cos(2 * M_PI * p / FTGP_PATH_POINTS);
        path[2 * p + 1] = 3.0 + 1.8 * sin(2 * M_PI * p / FTGP_PATH_POINTS);
    }
    long configs = 0, rejected = 0;
    for (int R : { 36, 90, 1080, 1083, 16384 })
        for (int cpe : { 1, 4, 8 })
            for (int n_envs : { 1, 7, 4096 })
                for (int fan_kind = 0; fan_kind < 3; ++fan_kind)        // 0: default, 1: a caller's point-symmetric fan, 2: a caller's irregular fan
                    for (int mode : { FTGP_LIDAR_RANGEFINDER, FTGP_LIDAR_FAKELIDAR })
                        for (int no_pairs = 0; no_pairs < 2; ++no_pairs) {
                            FtgpConfig cfg{};
                            cfg.abi_version = FTGP_ABI_VERSION;
                            cfg.n_envs = n_envs; cfg.cars_per_env = cpe; cfg.n_rays = R; cfg.spawn_mode = 1; cfg.dt = 0.01; cfg.lidar_mode = mode;
                            if (cpe == 8 && n_envs == 7) ftgp_tricycle_vehicle(&cfg.vehicle); else ftgp_default_vehicle(&cfg.vehicle);
                            cfg.track.width = W; cfg.track.height = H; cfg.track.words_per_row = wpr; cfg.track.bits = bits.data(); cfg.track.path = path.data();
                            cfg.track.px_size_x = cfg.track.px_size_y = 0.05;
                            std::vector<double> fan(2 * (size_t)R);
                            for (int j = 0; j < R; ++j) {
                                const double a = fan_kind == 2 ? 2 * M_PI * j / R + 0.3 * sin(j) / R : 2 * M_PI * j / R;
                                fan[2 * j] = cos(a); fan[2 * j + 1] = sin(a);
                                if (fan_kind == 1 && R % 2 == 0 && j >= R / 2) { fan[2 * j] = -fan[2 * (j - R / 2)]; fan[2 * j + 1] = -fan[2 * (j - R / 2) + 1]; }
                            }
                            if (fan_kind) cfg.fan_dirs = fan.data();
                            Switches sw;
                            sw.no_pairs = no_pairs != 0;
                            char label[160];
                            snprintf(label, sizeof label, "rays %d cars_per_env %d envs %d fan %d mode %d no_pairs %d", R, cpe, n_envs, fan_kind, mode, no_pairs);
                            if (validate(cfg, &cfg.track, 1, false, sw) != 0) { ++g_fail; printf("FAIL %s: validate: %s\n", label, ftgp_last_error()); continue; }
                            ++configs;
                            rejected += check(cfg, sw, label);
                        }
    {   // above 16384 rays: rejected before the shape
        FtgpConfig cfg{};
        cfg.n_envs = 1; cfg.cars_per_env = 1; cfg.n_rays = 16385; cfg.dt = 0.01;
        ftgp_default_vehicle(&cfg.vehicle);
        cfg.track.width = W; cfg.track.height = H; cfg.track.words_per_row = wpr; cfg.track.bits = bits.data(); cfg.track.path = path.data();
        cfg.track.px_size_x = cfg.track.px_size_y = 0.05;
        Plan pl;
        const int rc = plan(cfg, &cfg.track, &cfg.n_envs, 1, 256, Switches(), pl);
        printf("rays 16385: rejected (%d): %s\n", rc, ftgp_last_error());
        const char* label = "rays 16385";
        CHECK(rc == FTGP_ERR_ARG && strcmp(ftgp_last_error(), "n_rays above 16384 is not supported") == 0, "rc %d", rc);
    }
    for (int R : { 36, 1080 }) {   // FTGP_SCAN_EVERY_STEP: no window-only table, the two others as ever (outside the matrix: not counted as a configuration)
        FtgpConfig cfg{};
        cfg.abi_version = FTGP_ABI_VERSION;
        cfg.n_envs = 7; cfg.cars_per_env = 4; cfg.n_rays = R; cfg.spawn_mode = 1; cfg.dt = 0.01;
        ftgp_default_vehicle(&cfg.vehicle);
        cfg.track.width = W; cfg.track.height = H; cfg.track.words_per_row = wpr; cfg.track.bits = bits.data(); cfg.track.path = path.data();
        cfg.track.px_size_x = cfg.track.px_size_y = 0.05;
        Switches sw;
        Plan every, usual;
        const int rc0 = plan(cfg, &cfg.track, &cfg.n_envs, 1, 256, sw, usual);
        sw.scan_every_step = true;
        const int rc1 = plan(cfg, &cfg.track, &cfg.n_envs, 1, 256, sw, every);
        char label[64]; snprintf(label, sizeof label, "rays %d scan_every_step", R);
        CHECK(rc0 == 0 && rc1 == 0 && every.tasks == usual.tasks && every.tasks_win.empty() && every.tracks[0].P.win_tasks_per_car == 0 && usual.tracks[0].P.win_tasks_per_car > 0,
              "rc %d / %d, %d window-only tasks per car", rc0, rc1, every.tracks[0].P.win_tasks_per_car);
        printf("%s: %d window-only tasks per car, %d without the switch (of %d)\n", label, every.tracks[0].P.win_tasks_per_car, usual.tracks[0].P.win_tasks_per_car, usual.tracks[0].P.tasks_per_car);
    }
    {   // The window-only list's own cut (ftgp_window_cut.h) at the edges of its rule, with 1, 4 and 8 cars per env (outside the matrix: not counted
        // as configurations): want = pairs, single groups (a pair split at the tail counts as the pair it was), gathers, lanes of the last gather
        struct Fan { const char* name; int R, fan_kind; bool no_pairs; int pair_tail; bool first; int want[4]; };
        const Fan fans[] = {
            { "no full pair, two gathers", 128, 0, false, 2, false, { 0, 0, 2, 33 } },
            { "zones divide exactly, the gather is ray 0 alone", 512, 0, false, 2, false, { 2, 2, 1, 1 } },
            { "a rest on every zone", 520, 0, false, 2, false, { 2, 2, 1, 7 } },
            { "the headline's fan", 1080, 0, false, 2, false, { 4, 4, 1, 43 } },
            { "a caller's fan: singles only", 520, 2, false, 2, false, { 0, 6, 1, 7 } },
            { "FTGP_NO_PAIRS: singles only", 520, 0, true, 2, false, { 0, 6, 1, 7 } },
            { "at most 64 live rays: one gather", 80, 0, false, 2, false, { 0, 0, 1, 61 } },
            { "tail splits give way to the first table's task count", 640, 0, false, 2, false, { 2, 2, 2, 33 } },
            { "FTGP_PAIR_TAIL=0, a list longer than the first table: the first table again", 384, 0, false, 0, true, { 0, 0, 0, 0 } },
        };
        for (const Fan& f : fans)
            for (int cpe : { 1, 4, 8 }) {
                FtgpConfig cfg{};
                cfg.abi_version = FTGP_ABI_VERSION;
                cfg.n_envs = 7; cfg.cars_per_env = cpe; cfg.n_rays = f.R; cfg.spawn_mode = 1; cfg.dt = 0.01;
                ftgp_default_vehicle(&cfg.vehicle);
                cfg.track.width = W; cfg.track.height = H; cfg.track.words_per_row = wpr; cfg.track.bits = bits.data(); cfg.track.path = path.data();
                cfg.track.px_size_x = cfg.track.px_size_y = 0.05;
                std::vector<double> fan(2 * (size_t)f.R);
                for (int j = 0; j < f.R; ++j) { const double a = 2 * M_PI * j / f.R + 0.3 * sin(j) / f.R; fan[2 * j] = cos(a); fan[2 * j + 1] = sin(a); }
                if (f.fan_kind) cfg.fan_dirs = fan.data();
                Switches sw;
                sw.no_pairs = f.no_pairs; sw.pair_tail = f.pair_tail;
                char label[200]; snprintf(label, sizeof label, "window fan: rays %d cars_per_env %d (%s)", f.R, cpe, f.name);
                if (validate(cfg, &cfg.track, 1, false, sw) != 0 || check(cfg, sw, label, f.first) != 0) { ++g_fail; printf("FAIL %s: rejected: %s\n", label, ftgp_last_error()); continue; }
                Plan pl;
                plan(cfg, &cfg.track, &cfg.n_envs, 1, 256, sw, pl);
                const DeviceParams& P = pl.tracks[0].P;
                int got[4] = { 0, 0, 0, 0 }, halves = 0;
                for (int k = 0; k < P.win_tasks_per_car && !f.first; ++k) {
                    const int ent = P.win_group_order[k], kind = ent >> 16, j0 = ent & 0xffff;
                    if (kind == 3) ++got[2];
                    else if (kind == 1) ++got[0];
                    else {          // a single group of the cut, or one half of a pair split at the tail: both halves are there, a whole n/2 apart
                        bool other = false;
                        for (int q = 0; q < P.win_tasks_per_car; ++q) other = other || (P.win_group_order[q] >> 16 == 0 && abs((P.win_group_order[q] & 0xffff) - j0) == f.R / 2);
                        if (other && !f.no_pairs && !f.fan_kind) ++halves; else ++got[1];
                    }
                }
                got[0] += halves / 2;
                for (int k = 0; k < P.win_tasks_per_car && !f.first; ++k)      // lanes of the gather that is not full (the last of the cut)
                    if ((P.win_group_order[k] >> 16) == 3 && ((P.win_group_order[k] >> 7) & 127) == got[2] - 1) got[3] = P.win_group_order[k] & 127;
                CHECK(memcmp(got, f.want, sizeof got) == 0, "%d pairs, %d single groups, %d gathers, the last of %d lanes; want %d, %d, %d, %d", got[0], got[1], got[2], got[3],
                      f.want[0], f.want[1], f.want[2], f.want[3]);
            }
    }
    printf("digest=%016llx\n", (unsigned long long)g_digest.h);
    printf("plan_check: %ld configs, %ld rejected, %ld failures\n", configs, rejected, g_fail);
    return g_fail ? 1 : 0;
}
