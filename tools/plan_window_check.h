// The window-only table (plan_window_table), decoded as lidar_groups decodes it.  Of every car slot, every ray the drivers read -- ray 0 and rays
// eighth .. n - eighth - 1 -- is drawn exactly once and no other ray is drawn; ray 0 is drawn by a first group that carries the ray-0 flag; a
// delivered ray's window class is right (1 only where every ray of the group lies in the window, else 2); a pair or a single group is whole --
// 64 lanes, every one a live ray, a pair's on both sides; a gather's 64 entries (its runs expanded as gather_lanes does it) are rays below n or
// the sentinel 0xffff, the lanes in use first; ranks ascend, every car slot of a rank together, and a draw is the task win_group_order names
// at its rank; the list has no more tasks than the first table.  FTGP_TASK_MASKED is clear exactly on the pairs and single groups -- the PLAIN draws,
// which lidar_groups runs without a lane mask and delivers with one store: kind 0 or 1, never kind 2, 64 live rays a group, window class 1, no
// ray 0 -- and set on every gather.  A fan without an unread ray has the first table again (and its order), every entry marked FTGP_TASK_MASKED;
// first_table_ok: so may a fan whose own list would be longer than the first table (`times`: how often the first table draws a ray).
// Shared by plan_check.cpp, plan_tracks_check.cpp and plan_window_fans.cpp (after their CHECK macro).
#pragma once
static void check_window_table(const Plan& pl, const std::vector<int>& times, const char* label, bool every_step = false, bool first_table_ok = false)
{
    const DeviceParams& P = pl.tracks[0].P;
    const int R = P.n_rays, half = R / 2, cpb = P.cars_per_block, full = cpb * P.tasks_per_car, ntasks = cpb * P.win_tasks_per_car;
    if (every_step) { CHECK(ntasks == 0 && pl.tasks_win.empty(), "FTGP_SCAN_EVERY_STEP: %d window-only tasks, %zu ints", ntasks, pl.tasks_win.size()); return; }
    CHECK(pl.tasks_win.size() >= 4 * (size_t)ntasks && pl.tasks_win.size() % 4 == 0, "window-only table of %zu ints for %d tasks", pl.tasks_win.size(), ntasks);
    if (pl.tasks_win.size() < 4 * (size_t)ntasks || pl.tasks_win.size() % 4) return;
    const int n_gathers = (int)(pl.tasks_win.size() / 4) - ntasks;
    auto in_window = [&](int r) { return r >= P.eighth && r < R - P.eighth; };
    auto live = [&](int r) { return r == 0 || in_window(r); };
    bool dead = false;
    for (int j = 0; j < R; ++j) dead = dead || !live(j);
    CHECK(P.win_tasks_per_car >= 1 && P.win_tasks_per_car <= P.tasks_per_car, "%d window-only tasks per car of %d", P.win_tasks_per_car, P.tasks_per_car);
    // (the first table again: entry for entry, each marked FTGP_TASK_MASKED -- it has partial groups, kind 2 and every window class, so none of its
    // draws may take the window-only sweep's unmasked path)
    bool is_first = ntasks == full && n_gathers == 0;
    for (size_t i = 0; is_first && i < pl.tasks_win.size(); ++i) is_first = pl.tasks_win[i] == (pl.tasks[i] | (i % 4 == 0 ? FTGP_TASK_MASKED : 0));
    if (!dead || (first_table_ok && is_first)) {
        CHECK(is_first && memcmp(P.win_group_order, P.group_order, sizeof(int32_t) * (size_t)P.tasks_per_car) == 0, "the window-only table should be the first table, and is not");
        return;
    }
    std::vector<int> drawn((size_t)cpb * R, 0), zero_ok(cpb, 0);
    int marches = 0;
    for (int g = 0; g < ntasks; ++g) {
        const int32_t* d = &pl.tasks_win[4 * (size_t)g];
        const uint32_t x = (uint32_t)d[0];
        const int field = x & 0x3fff, kind = (x >> 14) & 3, c = (x >> 16) & 15, rank = d[1] >> 16, w0 = (x >> 20) & 3, w1 = (x >> 22) & 3, flag = (x >> 24) & 1;
        // ranks ascend, the car slots of a rank together; the draw is the task win_group_order names
        CHECK(c == g % cpb && rank == g / cpb && (x >> 26) == 0, "window draw %d: slot %d, rank %d, high bits %x", g, c, rank, x >> 26);
        // a PLAIN draw (FTGP_TASK_MASKED clear) runs without a lane mask and delivers with one store: kind 0 or 1 -- never kind 2 --, every group
        // wholly inside the window, no ray 0 (that all 64 lanes hold a live ray is checked lane by lane below); a gather is never plain
        const bool plain = (x & (uint32_t)FTGP_TASK_MASKED) == 0;
        CHECK(plain == (kind != 3) && kind != 2, "window draw %d: kind %d, plain %d", g, kind, (int)plain);
        if (plain) CHECK(kind <= 1 && w0 == 1 && w1 == (kind == 1 ? 1 : 0) && !flag && field + FTGP_WAVE <= (kind == 1 ? half : R),
                         "window draw %d: a plain draw of kind %d at ray %d with window classes %d / %d, ray-0 flag %d", g, kind, field, w0, w1, flag);
        if (!(c == g % cpb && rank == g / cpb)) continue;
        const int ent = P.win_group_order[rank];
        CHECK(kind == (ent >> 16) && field == (ent & 0xffff) && kind != 2, "window draw %d: kind %d, field %d, win_group_order[%d] = %x", g, kind, field, rank, ent);
        CHECK((d[1] & 0xffff) == c * (int)sizeof(LidarFrame) && d[2] == c * P.ranges_stride * 4 && d[3] == 4 * (c * P.win_floats + (P.eighth & 3) - P.eighth), "window draw %d: frame / row offsets", g);
        int map[FTGP_WAVE];                      // lane -> ray of the first group, 0xffff: none
        if (kind == 3) {
            const int lanes = field & 127, q = field >> 7;
            CHECK(lanes >= 1 && lanes <= FTGP_WAVE && q < n_gathers && w0 == 2 && w1 == 0, "window draw %d: gather %d of %d, %d lanes, window classes %d / %d", g, q, n_gathers, lanes, w0, w1);
            if (!(lanes <= FTGP_WAVE && q < n_gathers)) continue;
            const int32_t* r = &pl.tasks_win[4 * ((size_t)ntasks + q)];
            CHECK((r[0] >> 16) == 0 && (r[1] >> 16) >= 1 && (r[2] >> 16) >= (r[1] >> 16) && (r[3] >> 16) >= (r[2] >> 16) && (r[3] >> 16) <= FTGP_WAVE, "window draw %d: the runs' first lanes", g);
            for (int lane = 0; lane < FTGP_WAVE; ++lane) {       // gather_lanes()
                int dl = (int16_t)r[0];
                for (int k = 1; k < 4; ++k) if (lane >= (r[k] >> 16)) dl = (int16_t)r[k];
                map[lane] = lane < lanes ? lane + dl : 0xffff;
            }
        }
        else for (int lane = 0; lane < FTGP_WAVE; ++lane) {
            const int j = field + lane;
            map[lane] = j < (kind == 1 ? half : R) ? j : 0xffff;
            CHECK(map[lane] != 0xffff && live(j) && (kind != 1 || live(j + half)), "window draw %d: lane %d of a %s holds no live ray", g, lane, kind == 1 ? "pair" : "single group");
        }
        bool zero = false;
        for (int pass = 0; pass < (kind == 1 ? 2 : 1); ++pass) {
            ++marches;
            const int w = pass ? w1 : w0;
            for (int lane = 0; lane < FTGP_WAVE; ++lane) {
                if (map[lane] == 0xffff) continue;
                const int j = map[lane] + pass * half;
                CHECK(j >= 0 && j < R, "window draw %d: ray %d", g, j);
                if (j < 0 || j >= R) continue;
                ++drawn[(size_t)c * R + j];
                if (j == 0) { CHECK(pass == 0 && flag, "window draw %d: ray 0 in group %d without the ray-0 flag", g, pass); zero = true; zero_ok[c] = 1; }
                CHECK(w == 2 || (w == 1 && in_window(j)), "window draw %d: ray %d with window class %d", g, j, w);
            }
        }
        CHECK(zero == (flag != 0), "window draw %d: the ray-0 flag is %d, ray 0 drawn %d", g, flag, (int)zero);
        if (kind != 1) CHECK(w1 == 0, "window draw %d: second window class %d without a second group", g, w1);
    }
    long bad = 0, zero = 0, n_live = 0;
    for (size_t i = 0; i < drawn.size(); ++i) bad += drawn[i] != (live((int)(i % R)) ? 1 : 0);
    for (int c = 0; c < cpb; ++c) zero += zero_ok[c];
    for (int j = 0; j < R; ++j) n_live += live(j) ? 1 : 0;
    CHECK(bad == 0, "window-only table: %ld (car slot, ray): a read ray not drawn exactly once, or an unread ray drawn", bad);
    CHECK(zero == cpb, "window-only table: ray 0 drawn for %ld of %d car slots", zero, cpb);
    // as few marches as the live rays allow: every one full but the last gather's
    CHECK(marches == cpb * (int)((n_live + FTGP_WAVE - 1) / FTGP_WAVE), "window-only table: %d marches per car for %ld live rays", marches / cpb, n_live);
    (void)times;
}
