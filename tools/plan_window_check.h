// The window-only table (plan_window_table), decoded as lidar_groups decodes it: of every car slot, every ray the drivers read -- ray 0 and
// rays eighth .. n - eighth - 1 -- is drawn exactly once (`times`: or twice, where the first table draws it twice), no other ray is drawn, ray
// 0 is lane 0 of a first group that carries the ray-0 flag; each draw is a draw of the first table (its rank, its row offsets, its window
// classes), in the first table's order.
// Shared by plan_check.cpp and plan_tracks_check.cpp (after their CHECK macro).
#pragma once
static void check_window_table(const Plan& pl, const std::vector<int>& times, const char* label, bool every_step = false)
{
    const DeviceParams& P = pl.tracks[0].P;
    const int R = P.n_rays, half = R / 2, cpb = P.cars_per_block, full = cpb * P.tasks_per_car, ntasks = cpb * P.win_tasks_per_car;
    CHECK(pl.tasks_win.size() == 4 * (size_t)ntasks, "window-only table of %zu ints for %d tasks", pl.tasks_win.size(), ntasks);
    if (pl.tasks_win.size() != 4 * (size_t)ntasks) return;
    if (every_step) { CHECK(ntasks == 0, "FTGP_SCAN_EVERY_STEP: %d window-only tasks", ntasks); return; }
    auto live = [&](int r) { return r == 0 || (r >= P.eighth && r < R - P.eighth); };
    bool dead = false;
    for (int j = 0; j < R; ++j) dead = dead || !live(j);
    if (!dead) CHECK(ntasks == full && memcmp(pl.tasks_win.data(), pl.tasks.data(), sizeof(int32_t) * pl.tasks_win.size()) == 0, "no unread ray, but the window-only table is not the first table");
    else CHECK(P.win_tasks_per_car >= 1 && P.win_tasks_per_car <= P.tasks_per_car, "%d window-only tasks per car of %d", P.win_tasks_per_car, P.tasks_per_car);
    std::vector<int> drawn((size_t)cpb * R, 0), zero_ok(cpb, 0);
    int prev_rank = -1;
    for (int g = 0; g < ntasks; ++g) {
        const int32_t* d = &pl.tasks_win[4 * (size_t)g];
        const uint32_t x = (uint32_t)d[0];
        const int j0 = x & 0x3fff, kind = (x >> 14) & 3, c = (x >> 16) & 15, rank = d[1] >> 16, second = (x >> 26) & 1, trim = (x >> 25) & 1;
        CHECK(c == g % cpb && rank >= 0 && rank < P.tasks_per_car && kind != 3 && (x >> 27) == 0, "window draw %d: slot %d, rank %d, kind %d", g, c, rank, kind);
        if (!(c == g % cpb && rank >= 0 && rank < P.tasks_per_car)) continue;
        if (c == 0) { CHECK(rank > prev_rank, "window draw %d: rank %d after rank %d", g, rank, prev_rank); prev_rank = rank; }
        else CHECK(rank == prev_rank, "window draw %d: the car slots of a rank are not drawn together", g);
        // the draw of the first table it comes from
        const int32_t* a = &pl.tasks[4 * ((size_t)rank * cpb + c)];
        const uint32_t ax = (uint32_t)a[0];
        const int aj0 = ax & 0x3fff, akind = (ax >> 14) & 3;
        CHECK(d[1] == a[1] && d[2] == a[2] && d[3] == a[3], "window draw %d: frame / row offsets", g);
        if (second) CHECK(kind == 0 && akind == 1 && j0 == aj0 + half && ((x >> 20) & 3) == ((ax >> 22) & 3) && ((x >> 22) & 7) == 0, "window draw %d: second group of pair %d", g, rank);
        else if (kind != akind) CHECK(kind == 0 && akind == 1 && j0 == aj0 && aj0 + FTGP_WAVE <= half && ((x ^ ax) & (3u << 20 | 1u << 24)) == 0 && ((x >> 22) & 3) == 0, "window draw %d: first group of pair %d", g, rank);
        else CHECK(((x ^ ax) & ~(1u << 25)) == 0, "window draw %d differs from draw %d of the first table in more than bit 25", g, rank * cpb + c);
        bool unread = false;
        for (int pass = 0; pass < (kind == 1 ? 2 : 1); ++pass)
            for (int lane = 0; lane < FTGP_WAVE; ++lane) {
                int j; bool mine;
                if (kind == 2) { j = j0 + (lane & 31) + (lane >= 32 ? half : 0); mine = (lane & 31) < half - j0; }
                else { j = j0 + lane; mine = j < (kind == 1 ? half : R); }
                j += pass * half;
                if (!mine) continue;
                CHECK(j >= 0 && j < R, "window draw %d: ray %d", g, j);
                if (j < 0 || j >= R) continue;
                if (!live(j)) unread = true;
                if (trim && !live(j)) continue;
                ++drawn[(size_t)c * R + j];
                const int w = (x >> (20 + 2 * pass)) & 3;
                if (j == 0) { CHECK(pass == 0 && lane == 0 && ((x >> 24) & 1), "window draw %d: ray 0 in lane %d of group %d without the ray-0 flag", g, lane, pass); zero_ok[c] = 1; }
                if (j >= P.eighth && j < R - P.eighth) CHECK(w == 1 || w == 2, "window draw %d: ray %d with window class %d", g, j, w);
            }
        CHECK(unread == (trim != 0), "window draw %d: bit 25 is %d, unread rays %d", g, trim, (int)unread);
    }
    long bad = 0, zero = 0;
    for (size_t i = 0; i < drawn.size(); ++i) bad += drawn[i] != (live((int)(i % R)) ? times[i % R] : 0);
    for (int c = 0; c < cpb; ++c) zero += zero_ok[c];
    CHECK(bad == 0, "window-only table: %ld (car slot, ray): a read ray not drawn exactly once, or an unread ray drawn", bad);
    CHECK(zero == cpb, "window-only table: ray 0 drawn for %ld of %d car slots", zero, cpb);
}

