// Host harness: runs ftgp_create_tracks' plan (plan(): the batch's plan, every track's parameter block and tables, the workgroup table)
// and the layout of the two device images (layout_images, from made-up addresses) on the CPU, without a device, over synthetic track
// sets, ragged env counts, 1 / 3 / 8 cars per env and 90 / 1080 rays, in both workgroup orders, and checks what the multi-track step
// kernel relies on.
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -std=c++17 -x hip tools/plan_tracks_check.cpp -o /tmp/plan_tracks_check -ldl
#include "../ft_grandprix_amd/csrc/ftgp_api.hip"
#include "plan_digest.h"

#include <set>
#include <tuple>

static long g_fail = 0;
static Fnv g_digest;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAIL %s: ", label); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "plan_window_check.h"

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

static std::vector<int32_t> plan_in(int order, const FtgpConfig& cfg, const std::vector<FtgpTrack>& tr, const std::vector<int32_t>& counts, Plan& pl, int& rc)
{
    Switches sw;
    sw.track_order = order;
    rc = plan(cfg, tr.data(), counts.data(), (int)tr.size(), 256, sw, pl);
    return pl.wg;
}

// The two device images of a plan, laid out from made-up addresses: what the step kernel finds behind the workgroup table, task_tab and
// stage_img.  one: the plan has one track (no workgroup table in the image).
static void check_layout(const Plan& pl, const Images& im, const DeviceAddrs& a, bool one, const char* label)
{
    const int T = (int)pl.tracks.size();
    const DeviceParams& P = pl.tracks[0].P;
    const size_t head = FTGP_PARAMS_BYTES, wg_bytes = one ? 0 : sizeof(int32_t) * pl.wg.size(), tasks_bytes = sizeof(int32_t) * (pl.tasks.size() + pl.tasks_win.size());      // (all three tables)
    const size_t stage_bytes = (size_t)(P.off_cars - P.off_params) + 2 * (size_t)P.stage_cover, stride = (size_t)P.cover_kmax + 1;
    CHECK(im.blocks.size() == (size_t)T && im.blocks[0] == 0, "block offsets: %zu of them, the first at %zu", im.blocks.size(), im.blocks.empty() ? (size_t)0 : im.blocks[0]);
    CHECK(im.params.size() == head + wg_bytes + tasks_bytes + (size_t)(T - 1) * head + 16 && im.stage.size() == stage_bytes * T, "image sizes %zu / %zu", im.params.size(), im.stage.size());
    CHECK(memcmp(&im.P0, im.params.data(), sizeof im.P0) == 0, "track 0's finished block is not the head of the image");
    CHECK(memcmp(im.params.data() + head + wg_bytes, pl.tasks.data(), sizeof(int32_t) * pl.tasks.size()) == 0, "the task tables do not sit behind %s", one ? "the block" : "the workgroup table");
    CHECK(memcmp(im.params.data() + head + wg_bytes + sizeof(int32_t) * pl.tasks.size(), pl.tasks_win.data(), sizeof(int32_t) * pl.tasks_win.size()) == 0, "the window-only table does not sit behind the two task tables");
    if (one) CHECK(im.blocks == std::vector<size_t>{ 0 }, "one track: block offsets");
    else
        for (size_t b = 0; b < pl.wg.size(); b += 4) {       // the workgroup table: the plan's, each entry with its track's block offset
            int32_t w[4];
            memcpy(w, im.params.data() + head + sizeof(int32_t) * b, sizeof w);
            CHECK(w[1] == pl.wg[b + 1] && w[2] == pl.wg[b + 2] && w[3] == pl.wg[b + 3], "workgroup %zu: the image's entry is not the plan's", b / 4);
            CHECK(w[3] >= 0 && w[3] < T && (size_t)w[0] == im.blocks[(size_t)w[3]], "workgroup %zu: block offset %d of track %d", b / 4, w[0], w[3]);
        }
    for (int k = 0; k < T; ++k) {
        const Plan::Track& t = pl.tracks[(size_t)k];
        const size_t off = im.blocks[(size_t)k];
        CHECK(off % 16 == 0 && off + sizeof(DeviceParams) <= im.params.size() && (k == 0 || off >= head + wg_bytes + tasks_bytes), "track %d: block at %zu", k, off);
        if (off + sizeof(DeviceParams) > im.params.size()) continue;
        DeviceParams Q;
        memcpy(&Q, im.params.data() + off, sizeof Q);
        CHECK(Q.width == t.P.width && Q.height == t.P.height && Q.px_size_x == t.P.px_size_x && Q.plane256 == t.P.plane256, "track %d: the block at its offset is another track's", k);
        CHECK(Q.field == a.trk[(size_t)k].field && Q.edt == a.trk[(size_t)k].edt && Q.bits == a.trk[(size_t)k].bits && Q.nearbits == a.trk[(size_t)k].nearbits, "track %d: field / edt / bits / nearbits", k);
        CHECK(Q.path == a.path + 2 * FTGP_PATH_POINTS * (size_t)k && Q.spawn == a.spawn + 4 * FTGP_PATH_POINTS * (size_t)k, "track %d: path / spawn are not the shared buffers plus the track's stride", k);
        CHECK(Q.fan_dirs == a.fan && Q.veh_dev == a.veh && Q.ray_dir == a.ray && Q.cover_thr == a.cover && Q.cars == a.cars && Q.ranges == a.ranges && Q.steps == a.steps, "track %d: shared buffers", k);
        CHECK(Q.wg_metrics == a.wg_metrics && Q.wg_ticket == a.wg_ticket && Q.metrics_dev == a.metrics_dev && Q.metrics_host == a.metrics_host && Q.wg_metrics_host == a.wg_metrics_host, "track %d: metrics buffers", k);
        CHECK((const unsigned char*)Q.task_tab == a.params + head + wg_bytes, "track %d: task_tab", k);
        CHECK(Q.stage_img == a.stage + stage_bytes * k, "track %d: stage_img", k);
        // the staging image: head of the block | vehicle | centre-line | fan | cover tables of nidc and of fast
        const unsigned char* s = im.stage.data() + stage_bytes * k;
        CHECK(memcmp(s, &Q, offsetof(DeviceParams, veh)) == 0, "track %d: the stage image does not start with the head of the block", k);
        CHECK(memcmp(s + (P.off_veh - P.off_params), pl.veh.data(), pl.veh.size()) == 0, "track %d: staged vehicle image", k);
        CHECK(memcmp(s + (P.off_path - P.off_params), t.path.data(), sizeof(double) * t.path.size()) == 0 && t.path.size() == 2 * FTGP_PATH_POINTS, "track %d: staged centre-line", k);
        CHECK(memcmp(s + (P.off_ray - P.off_params), pl.ray.data(), sizeof(float) * pl.ray.size()) == 0, "track %d: staged fan", k);
        CHECK(memcmp(s + (P.off_cars - P.off_params), pl.cover.data(), sizeof(float) * stride) == 0, "track %d: staged cover table of nidc", k);
        CHECK(memcmp(s + (P.off_cars - P.off_params) + P.stage_cover, pl.cover.data() + stride, sizeof(float) * stride) == 0, "track %d: staged cover table of fast", k);
    }
}

// one configuration; returns 1 when the plan rejected it
static int check(const FtgpConfig& cfg, const std::vector<FtgpTrack>& tr, const std::vector<int32_t>& counts, const char* label)
{
    const int T = (int)tr.size(), cpe = cfg.cars_per_env, n_cars = cfg.n_envs * cpe;
    Plan pb, px; int rcb = 0, rcx = 0;
    const std::vector<int32_t> wb = plan_in(kOrderBlocks, cfg, tr, counts, pb, rcb), wx = plan_in(kOrderXcd, cfg, tr, counts, px, rcx);
    CHECK(rcb == rcx, "the orders disagree on the plan (%d / %d)", rcb, rcx);
    if (rcb) { printf("%s: rejected (%d): %s\n", label, rcb, ftgp_last_error()); return 1; }
    const int cpb = pb.tracks[0].P.cars_per_block;
    // each track's block and tables are those of a one-track plan of that track over the whole batch (same shape, sectors and fan)
    for (int t = 0; t < T; ++t) {
        Plan one;
        CHECK(plan(cfg, &tr[(size_t)t], &cfg.n_envs, 1, 256, Switches(), one) == 0, "one-track plan of track %d failed: %s", t, ftgp_last_error());
        if (one.tracks.size() != 1) continue;
        const Plan::Track& k = pb.tracks[(size_t)t], & k1 = one.tracks[0];
        CHECK(memcmp(&k.P, &k1.P, sizeof k.P) == 0, "track %d: the parameter block differs from its one-track plan's", t);
        CHECK(k.tab.bits == k1.tab.bits && k.tab.nearbits == k1.tab.nearbits && k.tab.runx == k1.tab.runx && k.tab.runy == k1.tab.runy, "track %d: tables differ", t);
        CHECK(k.spawn == k1.spawn && k.path == k1.path, "track %d: spawn table or centre-line differs", t);
        CHECK(one.tasks == pb.tasks && one.tasks_win == pb.tasks_win && one.ray == pb.ray, "track %d: the task tables or the fan differ", t);
        CHECK(one.n_wg == (cfg.n_envs * cpe + cpb - 1) / cpb, "track %d: %d workgroups in its one-track plan", t, one.n_wg);
        if (t == 0) {       // a one-track handle's images: the block, then the task tables
            const DeviceAddrs a = made_up_addrs(one);
            Images im;
            layout_images(one, a, im);
            check_layout(one, im, a, true, label);
        }
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
    for (const Plan* pl : { &pb, &px }) {
        {   // the window-only table: every ray the drivers read drawn once, no other, ray 0 present (`times`: a single group split off a short
            // pair runs on into the opposite half, as plan_check.cpp counts it)
            const DeviceParams& P = pl->tracks[0].P;
            const int R = P.n_rays, half = R / 2;
            std::vector<int> times((size_t)R, 1);
            bool pairs = false;
            for (int k = 0; k < P.tasks_per_car; ++k) pairs = pairs || (P.group_order[k] >> 16) != 0 || (P.group_order[k] & 0xffff) % FTGP_WAVE != 0;
            for (int k = 0; pairs && k < P.tasks_per_car; ++k) {
                const int j0 = P.group_order[k] & 0xffff;
                if ((P.group_order[k] >> 16) == 0 && j0 < half && j0 + FTGP_WAVE > half) for (int j = half; j < std::min(j0 + FTGP_WAVE, R); ++j) ++times[(size_t)j];
            }
            check_window_table(*pl, times, label);
        }
        const DeviceAddrs a = made_up_addrs(*pl);
        Images im;
        layout_images(*pl, a, im);
        check_layout(*pl, im, a, false, label);
        digest_plan(g_digest, *pl, im);
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
    printf("digest=%016llx\n", (unsigned long long)g_digest.h);
    printf("plan_tracks_check: %d configs, %d rejected, %ld failures\n", n, rejected, g_fail);
    return g_fail ? 1 : 0;
}
