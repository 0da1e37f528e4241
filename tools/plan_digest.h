// Shared by plan_check.cpp and plan_tracks_check.cpp (after their #include of ftgp_api.hip): made-up device addresses for layout_images and
// a 64-bit FNV-1a digest over everything the upload consumes of a plan -- every track's parameter block, bitmaps, run lengths and spawn
// table, the batch's tables, and both images laid out from those addresses.  Two builds that print the same digest plan the same handles.
#pragma once

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; } }
    template <class T> void vec(const std::vector<T>& v) { const uint64_t n = v.size(); bytes(&n, sizeof n); bytes(v.data(), sizeof(T) * v.size()); }
};

// distinct non-null addresses, the same for every configuration: buffer i at i * 2^32, a track's own buffers 2^28 apart; what the upload
// leaves null (the field or the distance transform and the fan, by lidar mode) is null here too
static DeviceAddrs made_up_addrs(const Plan& pl)
{
    auto at = [](uint64_t i, size_t k = 0) { return (uintptr_t)((i << 32) + ((uint64_t)k << 28)); };
    const bool fake = pl.tracks[0].P.lidar_mode == FTGP_LIDAR_FAKELIDAR;
    DeviceAddrs a;
    for (size_t k = 0; k < pl.tracks.size(); ++k)
        a.trk.push_back({ fake ? nullptr : (const uint16_t*)at(1, k), fake ? (const double*)at(2, k) : nullptr, (const uint32_t*)at(3, k), (const uint32_t*)at(4, k) });
    a.fan = fake ? (const double*)at(5) : nullptr; a.path = (const double*)at(6); a.spawn = (const double*)at(7); a.veh = (const void*)at(8);
    a.ray = (const float*)at(9); a.cover = (const float*)at(10); a.cars = (CarState*)at(11); a.ranges = (float*)at(12); a.steps = (int64_t*)at(13);
    a.wg_metrics = (double*)at(14); a.wg_ticket = (unsigned int*)at(15); a.metrics_dev = (double*)at(16); a.metrics_host = (double*)at(17);
    a.wg_metrics_host = (double*)at(18); a.params = (const unsigned char*)at(19); a.stage = (const unsigned char*)at(20);
    return a;
}

static void digest_plan(Fnv& f, const Plan& pl, const Images& im)
{
    const size_t T = pl.tracks.size();
    for (const Plan::Track& t : pl.tracks) {
        f.bytes(&t.P, sizeof t.P);
        f.vec(t.tab.bits); f.vec(t.tab.nearbits); f.vec(t.tab.runx); f.vec(t.tab.runy); f.vec(t.spawn);
    }
    f.vec(pl.ray); f.vec(pl.fan); f.vec(pl.cover); f.vec(pl.veh); f.vec(pl.tasks); f.vec(pl.tasks_win);
    if (T > 1) { f.vec(pl.wg); f.vec(pl.env_track); }      // (a one-track upload takes neither)
    f.bytes(&pl.n_wg, sizeof pl.n_wg);
    f.vec(im.params); f.vec(im.stage);
}
