// Host harness: runs ftgp_create_tracks' plan (plan_tracks: the batch's plan, every track's parameter block and tables, the workgroup
// table) on the CPU, without a device, over synthetic track sets, ragged env counts, 1 / 3 / 8 cars per env and 90 / 1080 rays, in both
// workgroup orders, and checks what the multi-track step kernel relies on.
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -std=c++17 -x hip tools/plan_tracks_check.cpp -o /tmp/plan_tracks_check -ldl
#include "../ft_grandprix_amd/csrc/ftgp_api.hip"

#include <set>
#include <tuple>

static long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAIL %s: ", label); printf(__VA_ARGS__); printf("\n"); } } while (0)

// a W x H image walled at its border with a block in the middle, a centre-line on an ellipse
struct SynthTrack {
    std::vector<uint32_t> bits;
    std::vector<double> path;
    FtgpTrack t{};
    SynthTrack(int W, int H, double px)
    {
        const int wpr = (W + 31) / 32;
        bits.assign((size_t)H * wpr, 0u);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const bool wall = x == 0 || y == 0 || x == W - 1 || y == H - 1 || (abs(x - W / 2) < W / 6 && abs(y - H / 2) < H / 6);
                if (wall) bits[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31);
            }
        path.resize(2 * FTGP_PATH_POINTS);
        for (int p = 0; p < FTGP_PATH_POINTS; ++p) {
            const double a = 2 * M_PI * p / FTGP_PATH_POINTS;
            path[2 * p] = 0.35 * W * px * cos(a); path[2 * p + 1] = 0.35 * H * px * sin(a);
        }
        t.width = W; t.height = H; t.words_per_row = wpr; t.bits = bits.data(); t.path = path.data();
        t.px_size_x = px; t.px_size_y = px; t.origin_x = -0.5 * W * px; t.origin_y = -0.5 * H * px;
    }
};

using Entry = std::tuple<int, int, int>;       // (track, first car, cars)

static std::vector<int32_t> plan_in(const char* order, const FtgpConfig& cfg, const std::vector<FtgpTrack>& tr, const std::vector<int32_t>& counts, Plan& pl, int& rc)
{
    setenv("FTGP_TRACK_ORDER", order, 1);
    rc = plan_tracks(cfg, tr.data(), counts.data(), (int)tr.size(), 256, pl);
    unsetenv("FTGP_TRACK_ORDER");
    return pl.wg;
}

// one configuration; returns 1 when the plan rejected it
static int check(const FtgpConfig& cfg, const std::vector<FtgpTrack>& tr, const std::vector<int32_t>& counts, const char* label)
{
    const int T = (int)tr.size(), cpe = cfg.cars_per_env, n_cars = cfg.n_envs * cpe;
    Plan pb, px; int rcb = 0, rcx = 0;
    const std::vector<int32_t> wb = plan_in("blocks", cfg, tr, counts, pb, rcb), wx = plan_in("xcd", cfg, tr, counts, px, rcx);
    CHECK(rcb == rcx, "the orders disagree on the plan (%d / %d)", rcb, rcx);
    if (rcb) { printf("%s: rejected (%d): %s\n", label, rcb, ftgp_last_error()); return 1; }
    const int cpb = pb.P.cars_per_block;
    // each track's block and tables are those of a one-track plan of that track over the whole batch (same shape, sectors and fan)
    for (int t = 0; t < T; ++t) {
        FtgpConfig c1 = cfg; c1.track = tr[(size_t)t];
        Plan one;
        CHECK(plan_create(c1, 256, one) == 0, "one-track plan of track %d failed: %s", t, ftgp_last_error());
        const Plan::Track* k = t ? &pb.more[(size_t)t - 1] : nullptr;
        const DeviceParams& Q = k ? k->P : pb.P;
        CHECK(memcmp(&Q, &one.P, sizeof Q) == 0, "track %d: the parameter block differs from its one-track plan's", t);
        const HostTables& tab = k ? k->tab : pb.tab;
        CHECK(tab.bits == one.tab.bits && tab.nearbits == one.tab.nearbits && tab.runx == one.tab.runx && tab.runy == one.tab.runy, "track %d: tables differ", t);
        CHECK((k ? k->spawn : pb.spawn) == one.spawn, "track %d: spawn table differs", t);
        CHECK(one.tasks == pb.tasks && one.ray == pb.ray, "track %d: the task tables or the fan differ", t);
    }
    // env -> track
    std::vector<int> env_track(cfg.n_envs, -1);
    for (int t = 0, e = 0; t < T; ++t) for (int i = 0; i < counts[(size_t)t]; ++i) env_track[(size_t)e++] = t;
    CHECK(pb.env_track.size() == (size_t)cfg.n_envs && std::equal(env_track.begin(), env_track.end(), pb.env_track.begin()), "env_track");
    // every car in exactly one workgroup; a workgroup's envs on its track; whole envs, at most cars_per_block cars
    std::set<Entry> sets[2];
    int nwg[2] = { 0, 0 };
    const std::vector<int32_t>* tabs[2] = { &wb, &wx };
    for (int o = 0; o < 2; ++o) {
        const std::vector<int32_t>& w = *tabs[o];
        const int n = (int)w.size() / 4;
        nwg[o] = n;
        std::vector<int> seen((size_t)n_cars, 0);
        for (int b = 0; b < n; ++b) {
            const int first = w[4 * (size_t)b + 1], cars = w[4 * (size_t)b + 2], t = w[4 * (size_t)b + 3];
            CHECK(w[4 * (size_t)b] == 0, "workgroup %d: the block offset is the upload's to fill in", b);
            CHECK(t >= 0 && t < T && cars >= 1 && cars <= cpb && first % cpe == 0 && cars % cpe == 0 && first >= 0 && first + cars <= n_cars,
                  "workgroup %d: track %d, cars [%d, %d)", b, t, first, first + cars);
            if (!(t >= 0 && t < T && first >= 0 && cars >= 1 && first + cars <= n_cars)) continue;
            for (int c = first; c < first + cars; ++c) { ++seen[(size_t)c]; CHECK(env_track[(size_t)(c / cpe)] == t, "workgroup %d (track %d) holds car %d of track %d", b, t, c, env_track[(size_t)(c / cpe)]); }
            sets[o].insert(Entry(t, first, cars));
        }
        for (int c = 0; c < n_cars; ++c) CHECK(seen[(size_t)c] == 1, "order %d: car %d sits in %d workgroups", o, c, seen[(size_t)c]);
        int want = 0;
        for (int t = 0; t < T; ++t) want += (counts[(size_t)t] * cpe + cpb - 1) / cpb;
        CHECK(n == want, "order %d: %d workgroups, want %d (each block its own, a ragged last one)", o, n, want);
    }
    CHECK(pb.n_wg == nwg[0] && px.n_wg == nwg[1], "n_wg");
    CHECK(sets[0] == sets[1], "the two orders cover different (track, workgroup) sets");
    // blocks order: track after track, cars ascending
    for (int b = 1; b < nwg[0]; ++b) CHECK(wb[4 * (size_t)b + 1] > wb[4 * (size_t)(b - 1) + 1], "blocks order: workgroup %d out of car order", b);
    // xcd order: each track owns a run of residues b % 8, the runs in track order, as many residues as its share of the workgroups
    {
        std::vector<int> lo(T, 99), hi(T, -1), nw(T, 0);
        std::vector<std::set<int>> res(T);
        for (int b = 0; b < nwg[1]; ++b) {
            const int t = wx[4 * (size_t)b + 3];
            res[(size_t)t].insert(b % 8); ++nw[(size_t)t];
            lo[(size_t)t] = std::min(lo[(size_t)t], b % 8); hi[(size_t)t] = std::max(hi[(size_t)t], b % 8);
        }
        for (int t = 0; t < T; ++t) {
            CHECK((int)res[(size_t)t].size() == hi[(size_t)t] - lo[(size_t)t] + 1, "xcd order: track %d's residues are not one run", t);
            const int share = (8 * nw[(size_t)t] + nwg[1] - 1) / nwg[1];
            CHECK((int)res[(size_t)t].size() <= share + 1, "xcd order: track %d holds %zu residues for %d of %d workgroups", t, res[(size_t)t].size(), nw[(size_t)t], nwg[1]);
            if (t) CHECK(lo[(size_t)t] >= hi[(size_t)t - 1], "xcd order: track %d's residues start before track %d's end", t, t - 1);
        }
    }
    printf("%s: ok, %d cars per workgroup, %d workgroups\n", label, cpb, nwg[0]);
    return 0;
}

int main()
{
    std::vector<SynthTrack> pool;
    pool.emplace_back(200, 150, 0.05); pool.emplace_back(320, 320, 0.025); pool.emplace_back(96, 400, 0.04); pool.emplace_back(257, 129, 0.03);
    pool.emplace_back(64, 64, 0.1); pool.emplace_back(500, 300, 0.02); pool.emplace_back(130, 131, 0.06); pool.emplace_back(33, 700, 0.01);
    std::vector<std::vector<int>> sets = { { 0, 1, 2, 3 }, { 4, 1, 6 }, { 0, 1, 2, 3, 4, 5, 6, 7 }, { 2, 5 } };
    std::vector<std::vector<int32_t>> splits4 = { { 37, 64, 5, 150 }, { 1, 1, 1, 1 }, { 1024, 1024, 1024, 1024 }, { 3, 700, 1, 97 } };
    std::vector<std::vector<int32_t>> splits3 = { { 37, 64, 5 }, { 2000, 1, 300 } };
    std::vector<std::vector<int32_t>> splits8 = { { 1, 2, 3, 4, 5, 6, 7, 8 }, { 600, 1, 77, 512, 9, 33, 100, 2 } };
    std::vector<std::vector<int32_t>> splits2 = { { 5, 4091 }, { 13, 13 } };
    int n = 0, rejected = 0;
    FtgpConfig base; memset(&base, 0, sizeof base);
    base.abi_version = FTGP_ABI_VERSION; base.lap_target = 10; base.dt = 0.004; base.seed = 7;
    ftgp_default_vehicle(&base.vehicle);
    for (const auto& ids : sets) {
        std::vector<FtgpTrack> tr;
        for (int i : ids) tr.push_back(pool[(size_t)i].t);
        const auto& splits = ids.size() == 4 ? splits4 : ids.size() == 3 ? splits3 : ids.size() == 8 ? splits8 : splits2;
        for (const auto& counts : splits)
            for (int cpe : { 1, 3, 8 })
                for (int rays : { 90, 1080 })
                    for (int mode : { FTGP_LIDAR_RANGEFINDER, FTGP_LIDAR_FAKELIDAR }) {
                        FtgpConfig cfg = base;
                        cfg.n_envs = 0; for (int32_t c : counts) cfg.n_envs += c;
                        cfg.cars_per_env = cpe; cfg.n_rays = rays; cfg.lidar_mode = mode; cfg.spawn_mode = cpe == 8 ? 1 : 0;
                        char label[160];
                        snprintf(label, sizeof label, "tracks %zu envs %d split %d.. cars_per_env %d rays %d mode %d", tr.size(), cfg.n_envs, counts[0], cpe, rays, mode);
                        ++n;
                        rejected += check(cfg, tr, counts, label);
                    }
    }
    printf("plan_tracks_check: %d configs, %d rejected, %ld failures\n", n, rejected, g_fail);
    return g_fail ? 1 : 0;
}
