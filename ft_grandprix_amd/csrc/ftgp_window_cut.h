// The cut of the window-only steps' rays into sweep tasks (plan_window_table; tools/sweep_model.cpp prices the same cut).  Host code only.
//
// The rays such a step marches are the ones the drivers read: ray 0 and rays [e, R - e), e = eighth.  A group-march costs what its slowest ray
// costs however few lanes it fills, so the cut makes as few marches as the live rays allow, every one of them full but the last:
//   pairs allowed (point-symmetric fan), h = R / 2:
//     sideways zone [e, h - e), whose opposites [h + e, R - e) are live too:  floor(n / 64) PAIRS of 64 + 64 rays
//     forward cone  [h - e, h + e), whose opposites nobody reads:             floor(n / 64) SINGLE groups of 64 consecutive rays
//     what is left -- ray 0, fewer than 64 rays of the zone, their opposites, fewer than 64 rays of the cone -- goes into GATHER tasks of at
//     most 64 lanes, runs of consecutive rays in consecutive lanes
//   no pairs: [e, R - e) in singles, its rest and ray 0 in a gather;  at most 64 live rays: one gather.
// Both zones leave their rest at their LOW end (side_low / cone_low: the other ends are what-ifs of tools/sweep_model.cpp, which prices all
// four under HIST=1; they lie within a wave-iteration of each other per car-step, DESIGN.md section 6 has the figures).
#pragma once
#include <utility>
#include <vector>

struct FtgpWindowCut {
    typedef std::pair<int, int> Run;                  // (first ray, rays)
    std::vector<int> pairs;                           // first ray of the first group of each pair
    std::vector<int> singles;                         // first ray of each single group
    std::vector<std::vector<Run>> gathers;            // per gather task: its runs in lane order (at most 4, 64 lanes in all)
};

inline FtgpWindowCut ftgp_window_cut(int R, int e, bool pairs_allowed, bool side_low = true, bool cone_low = true)
{
    FtgpWindowCut cut;
    std::vector<FtgpWindowCut::Run> rest;
    rest.push_back({ 0, 1 });
    const int h = R / 2, lo = e, hi = R - e;
    // a zone [a, b): whole groups of 64, the rest (at its low or its high end) to the gathers
    auto zone = [&](int a, int b, bool low, std::vector<int>& groups, bool opposite) {
        const int n = b - a, whole = n / 64, left = n - 64 * whole, first = low ? a + left : a;
        for (int k = 0; k < whole; ++k) groups.push_back(first + 64 * k);
        if (left) {
            const int r0 = low ? a : b - left;
            rest.push_back({ r0, left });
            if (opposite) rest.push_back({ r0 + h, left });
        }
    };
    if (1 + (hi - lo) <= 64) { if (hi > lo) rest.push_back({ lo, hi - lo }); }
    else if (pairs_allowed) {
        zone(lo, h - e, side_low, cut.pairs, true);
        zone(h - e, h + e, cone_low, cut.singles, false);
    }
    else zone(lo, hi, cone_low, cut.singles, false);
    // the rest, run by run, into gathers of at most 64 lanes (a run that does not fit goes on in the next gather)
    std::vector<FtgpWindowCut::Run> cur; int lanes = 0;
    for (FtgpWindowCut::Run r : rest)
        while (r.second > 0) {
            const int n = r.second < 64 - lanes ? r.second : 64 - lanes;
            cur.push_back({ r.first, n }); lanes += n; r.first += n; r.second -= n;
            if (lanes == 64) { cut.gathers.push_back(cur); cur.clear(); lanes = 0; }
        }
    if (!cur.empty()) cut.gathers.push_back(cur);
    return cut;
}
