// ftgp_api.hip -- implementation of the C-ABI of include/ftgp.h on top of the HIP kernels.
// Host code only owns resources and launches; there is no CPU compute path (no fallback).
#include <dlfcn.h>
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <hip/hip_ext.h>
#include "ftgp_kernels.hip"
#include "ftgp_window_cut.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* a = "")
{
    snprintf(g_err, sizeof g_err, fmt, a);
    return code;
}

int failf(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// the error of track k of a multi-track handle: its index in front of the message
int name_track(int code, int k)
{
    const std::string m(g_err);
    snprintf(g_err, sizeof g_err, "track %d: %s", k, m.c_str());
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            snprintf(g_err, sizeof g_err, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return FTGP_ERR_HIP;                                                                   \
        }                                                                                          \
    } while (0)

// ---- HIP resources, freed by their owners ------------------------------------------------------
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventFree { void operator()(hipEvent_t ev) const { (void)hipEventDestroy(ev); } };
struct StreamFree { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
template <class T> using DevBuf = std::unique_ptr<T, DevFree>;       // hipMalloc
template <class T> using HostBuf = std::unique_ptr<T, HostFree>;     // hipHostMalloc
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventFree>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamFree>;

template <class T> hipError_t dev_alloc(DevBuf<T>& b, size_t bytes) { void* p = nullptr; hipError_t r = hipMalloc(&p, bytes); b.reset(static_cast<T*>(p)); return r; }
template <class T> hipError_t dev_upload(DevBuf<T>& b, const void* src, size_t bytes)      // hipMalloc, then a copy from the host
{ hipError_t r = dev_alloc(b, bytes); return r != hipSuccess ? r : hipMemcpy(b.get(), src, bytes, hipMemcpyHostToDevice); }
template <class T> hipError_t dev_zeros(DevBuf<T>& b, size_t bytes, hipStream_t s)           // hipMalloc, then zeroed in stream order
{ hipError_t r = dev_alloc(b, bytes); return r != hipSuccess ? r : hipMemsetAsync(b.get(), 0, bytes, s); }
template <class T> hipError_t host_alloc(HostBuf<T>& b, size_t bytes, unsigned flags) { void* p = nullptr; hipError_t r = hipHostMalloc(&p, bytes, flags); b.reset(static_cast<T*>(p)); return r; }
hipError_t make_event(Event& ev, unsigned flags) { hipEvent_t p = nullptr; hipError_t r = hipEventCreateWithFlags(&p, flags); ev.reset(p); return r; }
hipError_t make_stream(Stream& s) { hipStream_t p = nullptr; hipError_t r = hipStreamCreateWithFlags(&p, hipStreamNonBlocking); s.reset(p); return r; }

// ---- RCCL, loaded lazily so that single-GPU use never touches it ------------------------------
struct Id128 { char internal[128]; };   // == ncclUniqueId (rccl.h:43)
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclFloat64 = 8;          // ncclFloat64 / ncclDouble (rccl.h ncclDataType_t)

Rccl g_rccl;

int load_rccl()
{
    if (g_rccl.lib) return 0;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(FTGP_ERR_COMM, "cannot load librccl.so: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void**, int, Id128, int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(FTGP_ERR_COMM, "librccl.so lacks an expected symbol%s");
    g_rccl.lib = h;
    return 0;
}

// the device copy of one track of a handle
struct TrackBufs {
    DevBuf<uint16_t> field; DevBuf<uint32_t> bits, nearbits;
    DevBuf<double> edt;               // FTGP_LIDAR_FAKELIDAR: distance transform
    int width = 0, height = 0;
    size_t block = 0;                 // byte offset of the track's parameter block in d_params (track 0: 0)
};

}  // namespace

// The members free themselves in reverse order of declaration, the streams last; ftgp_destroy synchronises both streams first.
struct FtgpEnv {
    DeviceParams P{};
    int device = 0;
    Stream stream, side;
    Event ev_start, ev_stop[2], ev_metrics, ev_gather;      // ev_stop: one per metrics slot
    bool timed = false;
    bool ext_launch = true;      // FTGP_LAUNCH_PLAIN switches it off (tools/launch_host.sh)
    bool last_roster = false;    // the newest launch ran the ROSTER instantiation
    // device buffers
    std::vector<TrackBufs> trk;       // per track: box field or distance transform, wall bitmaps (one entry for a one-track handle)
    DevBuf<double> d_path, d_spawn;   // [n_tracks][FTGP_PATH_POINTS][2] centre-lines, [n_tracks][FTGP_PATH_POINTS][4] spawn tables
    DevBuf<float> d_ray, d_cover; DevBuf<void> d_veh; DevBuf<unsigned char> d_stage; DevBuf<DeviceParams> d_params;
    DevBuf<CarState> d_cars; DevBuf<float> d_ranges; DevBuf<int64_t> d_steps;
    DevBuf<uint8_t> d_env_mask, d_car_mask; DevBuf<double> d_ctrl, d_pose;
    DevBuf<double> d_metrics, d_gather, d_wg_metrics; DevBuf<unsigned int> d_wg_ticket;
    DevBuf<double> d_fan;             // FTGP_LIDAR_FAKELIDAR: binary64 fan
    // multi-track handles (ftgp_create_tracks): one parameter block per track in d_params, the workgroup table behind track 0's
    int n_tracks = 1;
    DevBuf<int32_t> d_env_track;      // [n_envs] the track of every env (null with one track)
    int grid = 0;                     // workgroups of a step launch
    // This rank's metrics record lives in two slots (device memory for RCCL, pinned host memory for the caller) that successive
    // launches alternate between, so that the exchange of launch k's record can run beside launch k + 1.
    int cur_slot = 0;                    // slot of the most recent step launch (or of the record ftgp_metrics_kernel refreshed)
    bool launch_metrics_valid = false;   // slot cur_slot of d_metrics / h_metrics still describes the state (no reset / set_pose / ... since)
    HostBuf<double> h_metrics;        // pinned [2][FTGP_METRIC_DOUBLES]: THIS rank's records only (the gathered ones land in h_gather)
    double* h_metrics_dev = nullptr;  // the same buffer as the device sees it: the step kernel's epilogue writes straight into it
    HostBuf<double> h_gather;         // pinned [world][FTGP_METRIC_DOUBLES]: landing buffer of the all-gather
    HostBuf<double> h_wg_metrics;     // pinned [2][workgroups][FTGP_METRIC_DOUBLES]: the workgroups' partial records of a launch (one rank, no communicator:
                                      // nothing on the device needs the launch's record, the host adds the partial records up -- collect_slot())
    bool slot_partial[2] = { false, false };   // the record of that slot's launch is in h_wg_metrics (partial records), not in h_metrics
    bool gather_open = false;         // ftgp_metrics_allgather_begin without its _end
    int gather_slot = 0;              // the slot that exchange reads
    hipEvent_t gather_event = nullptr;   // what its _end waits for: ev_gather (side stream / metrics kernel) or the slot's own ev_stop
    bool gather_held = false;         // one rank: the record was copied to `held` because a later launch was about to reuse its slot
    double held[FTGP_METRIC_DOUBLES] = { 0 };
    DevBuf<int32_t> d_prog; DevBuf<double> d_core;
    std::vector<int32_t> h_prog; std::vector<double> h_core;
    bool rows_valid = false;          // h_prog / h_core mirror the device state (cleared by every call that changes it)
    bool multi = false;
    HostBuf<int32_t> h_tables;        // pinned [2][FTGP_MAX_CARS_PER_BLOCK]: the user's roster (mirror of P.car_policy), the device-io slot table
    int table_on_device = 0;          // which of the two the params block holds (-1: neither); only a FTGP_POLICY_PER_CAR launch reads it
    // device I/O (ftgp_device_io_config / ftgp_step_device): everything the device step keeps on the host
    struct DeviceStep {
        bool ready = false;               // ftgp_device_io_config has run
        DeviceIoArgs io{};                // the episode rules and the slot table; the buffers are filled in per call
        int repeat = 1;
        DevBuf<int32_t> d_prev_abs;
        Event ev_in, ev_out;              // the fences between the caller's stream and the handle's
        DeviceSignalArgs sig{};           // ftgp_device_io_signals (the buffers and what depends on them are filled in per call)
        bool sig_default = true;          // the defaults: a call without state buffers launches ftgp_io_finish_kernel
        bool con_on = false;              // ftgp_device_io_contacts: a call evaluates the contact rows and goes through ftgp_io_finish_signals_kernel
        FtgpDeviceContacts con{};         // the contact rules while con_on
        DevBuf<float> d_contact;          // [n_cars][FTGP_CONTACT_FLOATS] every car's contact row, allocated on first use
        bool frame_on = false;            // ftgp_device_io_frame: a call evaluates the frame rows and goes through ftgp_io_finish_signals_kernel
        FtgpDeviceFrame frame{};          // n_ahead, stride and the reward rule while frame_on
        DevBuf<float> d_frame;            // [n_cars][FTGP_FRAME_FIXED + 2 * FTGP_MAX_LOOKAHEAD] floats, rows packed at the width in use; allocated on first use.
                                          // Scratch of one call: ftgp_get_frames packs rows of ITS width in here too, which is safe only because every device
                                          // step rewrites the buffer on the handle's stream before its finish kernel reads it -- nothing may be kept in it across calls
        DevBuf<double> d_frame_s;         // [2][n_cars] s before and after a call's steps (dense progress)
        DevBuf<int32_t> d_frame_flag;     // [2][n_cars] the flags that go with them
        bool rivals_on = false;           // ftgp_device_io_rivals: a call evaluates the rival rows and goes through ftgp_io_finish_signals_kernel
        FtgpDeviceRivals rivals{};        // n_rivals and the place weight while rivals_on
        DevBuf<float> d_rival;            // [n_cars][FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * FTGP_MAX_RIVALS] floats, rows packed at the width in use; scratch of one
                                          // call like d_frame, allocated on first use
        DevBuf<int32_t> d_frame_c;        // [2][n_cars] the nearest points that go with d_frame_s (the rival rows' race progress)
        DevBuf<int32_t> d_place0;         // [n_cars] the places when the call began (place reward)
        DevBuf<float> d_collect_obs;      // [n_cars][n_rays] ftgp_collect_device: where the obs rows of its device steps go (not part of the record); allocated on first use
        struct { const void* p; size_t bytes; } checked[32] = {};     // device buffers found valid (hipPointerGetAttributes), replaced round robin
        int checked_next = 0;
    } ds;
    // spawn rule (ftgp_set_spawn_rule)
    std::vector<double> start_table;  // [n_tracks][FTGP_PATH_POINTS][6] x, y, qw, qz, clear_left, clear_right: the plan's (ftgp_get_start_table)
    const FtgpSpawnDev* rule = nullptr;      // what the reset paths are handed: d_rule while a rule is set, null without one
    DevBuf<FtgpSpawnDev> d_rule; DevBuf<int32_t> d_start, d_n_start; DevBuf<double> d_clear; DevBuf<int64_t> d_episodes;      // allocated by the first rule
    // per-car dynamics (ftgp_set_dynamics)
    DevBuf<double> d_dyn;             // [n_cars][FTGP_DYN_RECORD] records, then the rejected counter; allocated by the first setter call (ensure_dynamics)
    bool dyn_on = false;              // step launches run the DYN instantiations
    DynArgs dyn{};                    // the handle's own row and the wheel-load rule (the buffers are filled in per call)
    DevBuf<double> d_dyn_rows;        // [n_cars][FTGP_DYN_DOUBLES] landing buffer of the host setter, allocated on first use
    // network drivers (ftgp_set_net): the two tables the kernels read, and one NetSlot per slot with everything else (below)
    DevBuf<NetDev> d_nets;            // [FTGP_MAX_NETS] the policies' records; allocated by the first setter call (ensure_nets)
    bool last_net = false;            // the newest launch ran a NET instantiation
    // the value nets' records are read by the VALUE instantiations of ftgp_collect_act_kernel alone, so they have a table of their own and the
    // parameter blocks know nothing of them
    DevBuf<NetDev> d_vnets;           // [FTGP_MAX_NETS] NetDev-shaped records: the layers, the output map in out_scale[0] / out_offset[0], params; allocated by the first ftgp_set_value_net
    // a trainer (ftgp_train_begin): nothing of it exists on a handle that never asked for one
    struct Trainer {
        bool on = false;
        FtgpTrainDesc desc{};
        int64_t t = 0;                    // Adam steps taken
        int n[2] = { 0, 0 };              // n_floats of the policy and of the value net (the library's layout)
        DevBuf<float> grad, m, v;         // [n[0] + n[1]] the policy's, then the value net's
        DevBuf<float> part;               // [FTGP_TRAIN_MAX_WG][n[0] + n[1]] the workgroups' partial sums
        DevBuf<float> stats;              // [2 * FTGP_TRAIN_MAX_WG + 1][FTGP_TRAIN_STATS] the workgroups' partial stats, the stats of the newest gradient, the workgroups' binary64 sums (four doubles each)
        DevBuf<int32_t> sync;             // the gradient's non-finite flag, the reduce kernel's ticket
    };
    // One network slot: the policy (ftgp_set_net), and what hangs on it -- a population (ftgp_set_net_population), a value net
    // (ftgp_set_value_net), a trainer (ftgp_train_begin).
    struct NetSlot {
        NetDev net{};                     // host mirror of the slot's record in d_nets (defined = 0: an empty slot)
        FtgpNetDesc desc{};               // the description as the caller gave it (ftgp_get_net)
        FtgpNetFrame frame{};             // ... and the frame inputs (ftgp_get_net_frame); zeros = none
        FtgpNetRivals rivals{};           // ... and the rival inputs (ftgp_get_net_rivals); zeros = none
        DevBuf<float> d_params;           // the slot's single parameter set in the library's layout
        int pop_members = 0;              // > 0: the slot carries a population, and its record's params and env_member point here
        DevBuf<float> d_pop_params;       // [pop_members] parameter sets in the library's layout, net_member_stride(n_floats) floats apart
        DevBuf<int32_t> d_pop_map;        // [n_envs] the member of every env
        NetDev vnet{};                    // host mirror of the value net's record in d_vnets (defined = 0: none)
        FtgpValueDesc vdesc{};            // its description as the caller gave it (ftgp_get_value_net)
        DevBuf<float> d_vparams;          // its parameters in the library's layout
        Trainer trainer;
        // What ends with what.  A trainer steps the slot's single parameter set and its value net, so it ends when a population takes the
        // set's place and whenever the value net is set or cleared.  The value net reads the policy's inputs, and a population is sets of the
        // policy's shape, so both end -- and the trainer with them -- when the policy is defined anew or cleared.  Each call releases device
        // buffers: the setters make it once the stream is idle and the slot's new record is on the device.
        void end_trainer() { trainer = Trainer{}; }
        void end_value() { vnet = NetDev{}; vdesc = FtgpValueDesc{}; d_vparams.reset(); end_trainer(); }
        void end_population() { pop_members = 0; d_pop_params.reset(); d_pop_map.reset(); }
    } slots[FTGP_MAX_NETS];
    // env states (ftgp_save_envs_device / ftgp_load_envs_device)
    std::vector<uint64_t> track_fp;   // [n_tracks] the tracks' fingerprints (include/ftgp.h), folded at create
    DevBuf<EnvStateAux> d_state_aux;  // the handle's own dynamics record, the rejected counter, the fingerprints; allocated by the first save or load
    // comm
    void* comm = nullptr; int rank = 0, world = 1;
};

namespace {

constexpr int kCoreDoubles = 16;     // row of ftgp_pack_kernel

// exact chessboard distance transform of a W x H occupancy image (two raster sweeps over a padded image)
void chessboard_dt(const std::vector<uint8_t>& occ, int W, int H, std::vector<int>& out)
{
    const int S = W + 2;
    std::vector<int> d((size_t)S * (H + 2), 1 << 20);
    auto at = [&](int x, int y) -> int& { return d[(size_t)(y + 1) * S + (x + 1)]; };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) if (occ[(size_t)y * W + x]) at(x, y) = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int n = std::min(std::min(at(x - 1, y), at(x - 1, y - 1)), std::min(at(x, y - 1), at(x + 1, y - 1))) + 1;
            if (n < at(x, y)) at(x, y) = n;
        }
    for (int y = H - 1; y >= 0; --y)
        for (int x = W - 1; x >= 0; --x) {
            const int n = std::min(std::min(at(x + 1, y), at(x + 1, y + 1)), std::min(at(x, y + 1), at(x - 1, y + 1))) + 1;
            if (n < at(x, y)) at(x, y) = n;
        }
    out.resize((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) out[(size_t)y * W + x] = at(x, y);
}

// Host-side inputs of the sector box field (the boxes themselves are searched on the GPU, ftgp_box_field_kernel) and the
// bitmaps of the wall contact.
struct HostTables {
    std::vector<uint8_t> wall;        // [H][W] 1 = wall
    std::vector<uint16_t> runx, runy; // [2][H][W] wall-free run lengths along +x / -x and +y / -y (0 on walls, 65535 = beyond the image)
    std::vector<uint32_t> bits, nearbits;   // [H][wpr], padding bits clear
};

void build_tables(const FtgpTrack& t, int reach, HostTables& g)
{
    const int W = t.width, H = t.height, wpr = t.words_per_row;
    g.wall.assign((size_t)W * H, 0);
    g.bits.assign((size_t)H * wpr, 0u); g.nearbits.assign((size_t)H * wpr, 0u);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if ((t.bits[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u) {
                g.wall[(size_t)y * W + x] = 1; g.bits[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31);
            }
    std::vector<int> dpx;
    chessboard_dt(g.wall, W, H, dpx);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (dpx[(size_t)y * W + x] <= reach) g.nearbits[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31);
    const size_t plane = (size_t)W * H;
    g.runx.assign(2 * plane, 0); g.runy.assign(2 * plane, 0);
    for (int y = 0; y < H; ++y) {
        int r = 65535;
        for (int x = W - 1; x >= 0; --x) { r = g.wall[(size_t)y * W + x] ? 0 : std::min(65535, r + 1); g.runx[(size_t)y * W + x] = (uint16_t)r; }
        r = 65535;
        for (int x = 0; x < W; ++x) { r = g.wall[(size_t)y * W + x] ? 0 : std::min(65535, r + 1); g.runx[plane + (size_t)y * W + x] = (uint16_t)r; }
    }
    for (int x = 0; x < W; ++x) {
        int r = 65535;
        for (int y = H - 1; y >= 0; --y) { r = g.wall[(size_t)y * W + x] ? 0 : std::min(65535, r + 1); g.runy[(size_t)y * W + x] = (uint16_t)r; }
        r = 65535;
        for (int y = 0; y < H; ++y) { r = g.wall[(size_t)y * W + x] ? 0 : std::min(65535, r + 1); g.runy[plane + (size_t)y * W + x] = (uint16_t)r; }
    }
}

inline int pad16(size_t n) { return (int)((n + 15) & ~(size_t)15); }

// nidc.py:57,93-99 exactly as the driver evaluates it (binary64, libm): points covered by a disparity whose closer sample is d
int cover_count_host(double width, double rpp, double close_dist)
{
    const double angle = 2 * atan(width / (2 * close_dist));
    const double cnt = ceil(angle / rpp);
    return (cnt > 2147483000.0) ? 2147483000 : (cnt < -2147483000.0 ? -2147483000 : (int)cnt);
}

// thr[k], k = 1 .. kmax: the largest positive binary32 sample whose count is still >= k (the count never increases with the
// sample); thr[0] = the count of a sample of exactly 0.  Found by bisection over the bit patterns of the positive floats.
void build_cover_table(double car_width, int n_rays, int kmax, float* thr)
{
    const double width = (car_width / 2) * (1 + 300.0 / 100);       // nidc.py:93
    const double rpp = (2 * M_PI) / (double)n_rays;                 // nidc.py:121
    auto num = [&](uint32_t bits) { float f; memcpy(&f, &bits, 4); return cover_count_host(width, rpp, (double)f); };
    thr[0] = (float)cover_count_host(width, rpp, 0.0);
    for (int k = 1; k <= kmax; ++k) {
        uint32_t lo = 1u, hi = 0x7f7fffffu;                         // num(lo) >= k by the choice of kmax; num(hi) may be < k
        if (num(hi) >= k) { memcpy(&thr[k], &hi, 4); continue; }
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (num(mid) >= k) lo = mid; else hi = mid; }
        memcpy(&thr[k], &lo, 4);
    }
}

// LDS layout for `cpb` cars and `wpb` waves per workgroup; returns the total
int lds_layout(DeviceParams& P, int cpb, int wpb)
{
    int o = 0;
    P.off_params = o; o += pad16(offsetof(DeviceParams, veh));              // the head of the block: what the step kernel reads
    P.off_veh = o;    o += pad16(sizeof(VehLds));
    P.off_path = o;   o += pad16(sizeof(double) * 2 * FTGP_PATH_POINTS);
    P.off_ray = o;    o += pad16(sizeof(float) * 2 * (size_t)P.n_rays);
    P.off_cars = o;   o += cpb * (int)sizeof(CarCore);
    P.off_frame = o;  o += 2 * cpb * (int)sizeof(LidarFrame);      // double-buffered by step parity
    if (P.cars_per_env > 1) o += 2 * cpb * FTGP_PAIR_STRIDE * (int)sizeof(PairCull);   // env-mate records, right behind the frames
    P.off_steps = o;  o += pad16((size_t)cpb * sizeof(int64_t));
    P.off_scan = o;   o += 2 * cpb * P.win_floats * (int)sizeof(float);   // double-buffered by step parity
    P.off_list = o;   o += std::min(cpb, wpb) * FTGP_WAVE * (int)sizeof(int);                 // driver scratch: wave c runs the driver of car c
    P.off_pool = o;   o += 32;
    P.off_k1 = o;     o += cpb * (FTGP_FORCE_TERMS * 24 + 4 * 8 + 104 + (P.cars_per_env > 1 ? FTGP_PAIR_STRIDE * 24 : 0));   // K1 staging: force terms | new wheel spins | new state [| contact sums per env-mate]
    P.mmask_stride = pad16((size_t)2 * (size_t)((P.n_rays + FTGP_WAVE - 1) / FTGP_WAVE + 2));      // two groups per task, never more tasks than groups of 64 rays + 2
    P.off_mmask = o;  if (P.cars_per_env > 1) o += 2 * cpb * P.mmask_stride;              // env-mate visibility masks, double-buffered by step parity
    P.stage_cover = pad16(sizeof(float) * (size_t)(P.cover_kmax + 1));
    P.off_cover = o;  o += 2 * P.stage_cover;                                               // cover-count thresholds of the launch's driver (FTGP_POLICY_PER_CAR: of both, nidc's first)
    P.lds_bytes = o;
    P.cars_per_block = cpb; P.waves_per_block = wpb;
    return o;
}

// the device probe of the entries that open a device: there is one (no CPU fallback) and `id` names it; it is made current
int open_device(int id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(FTGP_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback%s");
    if (id < 0 || id >= ndev) return fail(FTGP_ERR_ARG, "device_id out of range%s");
    HIP_TRY(hipSetDevice(id));
    return 0;
}

// The FTGP_* environment switches (INTEGRATION.md has the table).  ftgp_create / ftgp_create_tracks read them once, here, and hand them
// down: the plan is a function of its arguments.
enum { kOrderBlocks = 0, kOrderXcd = 1 };     // FTGP_TRACK_ORDER (plan_workgroups)
struct Switches {
    bool no_pairs = false, group_order_plain = false, puck_test = false, no_fused_metrics = false, no_host_sum = false, launch_plain = false, verbose = false;
    bool scan_every_step = false;     // FTGP_SCAN_EVERY_STEP: no window-only steps (plan_window_table)
    int sectors_rt = 0;               // 8, 16, 32 or 64 direction sectors; 0: by car count (sector_count)
    int waves_per_block = 16;         // 1 .. 16
    int cars_per_block = 0;           // as given: plan_shape takes it where it is in range, rounded down to whole envs
    int lds_cap = 80 * 1024;          // bytes, of 16 .. 160 KiB
    int pair_tail = 2;
    int track_order = kOrderXcd;
};

Switches read_switches()
{
    Switches sw;
    sw.no_pairs = getenv("FTGP_NO_PAIRS") != nullptr; sw.group_order_plain = getenv("FTGP_GROUP_ORDER_PLAIN") != nullptr; sw.puck_test = getenv("FTGP_PUCK_TEST") != nullptr;
    sw.no_fused_metrics = getenv("FTGP_NO_FUSED_METRICS") != nullptr; sw.no_host_sum = getenv("FTGP_NO_HOST_SUM") != nullptr;
    sw.launch_plain = getenv("FTGP_LAUNCH_PLAIN") != nullptr; sw.verbose = getenv("FTGP_VERBOSE") != nullptr;
    if (const char* sv = getenv("FTGP_SCAN_EVERY_STEP")) sw.scan_every_step = atoi(sv) != 0;
    if (const char* sv = getenv("FTGP_SECTORS_RT")) { const int c = atoi(sv); if (c == 8 || c == 16 || c == 32 || c == 64) sw.sectors_rt = c; }
    if (const char* sv = getenv("FTGP_WAVES_PER_BLOCK")) { const int c = atoi(sv); if (c >= 1 && c <= 16) sw.waves_per_block = c; }
    if (const char* sv = getenv("FTGP_CARS_PER_BLOCK")) sw.cars_per_block = atoi(sv);
    if (const char* sv = getenv("FTGP_LDS_CAP_KB")) { const int c = atoi(sv); if (c >= 16 && c <= 160) sw.lds_cap = c * 1024; }
    if (const char* sv = getenv("FTGP_PAIR_TAIL")) sw.pair_tail = atoi(sv);
    if (const char* sv = getenv("FTGP_TRACK_ORDER")) sw.track_order = strcmp(sv, "blocks") == 0 ? kOrderBlocks : kOrderXcd;
    return sw;
}

// Direction sectors of the box field: more slope slices mean fewer march iterations and a larger field.  A large batch is bound by
// throughput and by what of the field its cars keep in the 4-MiB L2s (16 sectors: 32 bytes per pixel); a small one by the latency of
// its longest rays (64 sectors); 16384 cars (config 5) do best with 8.  Measured: profiles/round4/ab_sectors.log.  Results do not depend on the choice.
int sector_count(const FtgpConfig& cfg, const Switches& sw)
{
    const long cars_total = (long)cfg.n_envs * cfg.cars_per_env;
    return sw.sectors_rt ? sw.sectors_rt : cars_total >= 8192 ? 8 : cars_total >= 2048 ? 16 : 64;
}

// ftgp_create, step 1: the checks of the configuration with its tracks (no device call).  named: an error of a track names its index
// (ftgp_create_tracks).
int validate(const FtgpConfig& cfg, const FtgpTrack* tracks, int n_tracks, bool named, const Switches& sw)
{
    if (cfg.abi_version != FTGP_ABI_VERSION) return fail(FTGP_ERR_ARG, "abi version mismatch%s");
    if (cfg.n_envs < 1 || cfg.cars_per_env < 1 || cfg.cars_per_env > 8 || cfg.n_rays < 1) return fail(FTGP_ERR_ARG, "bad n_envs / cars_per_env / n_rays%s");
    if (cfg.spawn_mode == 0 && (cfg.cars_per_env + 4) * 2 + 1 >= FTGP_PATH_POINTS) return fail(FTGP_ERR_ARG, "too many cars for the reference spawn rule%s");
    auto bad = [&](int k, int rc) { return named ? name_track(rc, k) : rc; };
    const uint64_t n_sectors = (uint64_t)sector_count(cfg, sw);
    for (int k = 0; k < n_tracks; ++k) {
        const FtgpTrack& t = tracks[k];
        if (t.width < 1 || t.height < 1 || !t.bits || !t.path || t.words_per_row < (t.width + 31) / 32) return bad(k, fail(FTGP_ERR_ARG, "bad track%s"));
        if (t.width > 8192 || t.height > 8192) return bad(k, fail(FTGP_ERR_ARG, "images above 8192 pixels are not supported%s"));
        // the march addresses the field with a 32-bit byte offset
        if ((uint64_t)ftgp_plane256(t.width, t.height) * 256u * n_sectors > 0xFFFFFFFFull)
            return bad(k, fail(FTGP_ERR_ARG, "track image too large: the sector box field (2 bytes per pixel and direction sector) must stay below 4 GiB%s"));
    }
    if (cfg.env_base < 0) return fail(FTGP_ERR_ARG, "env_base < 0%s");
    if (cfg.lidar_mode != FTGP_LIDAR_RANGEFINDER && cfg.lidar_mode != FTGP_LIDAR_FAKELIDAR) return fail(FTGP_ERR_ARG, "unknown lidar_mode%s");
    if (!(cfg.dt > 0.0)) return fail(FTGP_ERR_ARG, "bad dt / pixel size%s");
    for (int k = 0; k < n_tracks; ++k)
        if (!(tracks[k].px_size_x > 0.0) || !(tracks[k].px_size_y > 0.0)) return bad(k, fail(FTGP_ERR_ARG, "bad dt / pixel size%s"));
    const FtgpVehicle& v = cfg.vehicle;
    if (!(v.contact_radius > 0.0) || !(v.mass > 0.0) || !(v.izz > 0.0) || (v.kind != FTGP_VEHICLE_MUSHR && v.kind != FTGP_VEHICLE_TRICYCLE))
        return fail(FTGP_ERR_ARG, "bad vehicle%s");
    if (cfg.bubble_wrap && !(v.softener_radius > 0.0)) return fail(FTGP_ERR_ARG, "bubble_wrap needs vehicle.softener_radius > 0%s");
    return 0;
}

// ftgp_create, step 2: the plan -- everything that fixes what the step kernel does; host arithmetic only (no HIP call)
struct Plan {
    struct Track {
        DeviceParams P = DeviceParams();  // the batch's parameter block with the track's own values (plan_track_params).  Value-initialised
                                          // (padding bytes zero: the block is uploaded as it lies); every pointer null
        HostTables tab;               // bitmaps and run lengths of the track (build_tables)
        std::vector<double> spawn;    // [FTGP_PATH_POINTS][4] x, y, qw, qz
        std::vector<double> clear;    // [FTGP_PATH_POINTS][2] wall clearance to the left / right of the spawn table's points (ftgp_start_table)
        std::vector<double> path;     // [FTGP_PATH_POINTS][2] the caller's centre-line
    };
    std::vector<Track> tracks;        // one per track of the handle (ftgp_create: one)
    std::vector<float> ray;           // [n_rays][2] binary32 fan, zero-padded to 16 bytes (DeviceParams::ray_dir)
    std::vector<double> fan;          // [n_rays][2] binary64 fan (FAKELIDAR: DeviceParams::fan_dirs)
    std::vector<float> cover;         // cover-count thresholds of nidc, then of fast, cover_kmax + 1 each (+ padding)
    std::vector<unsigned char> veh;   // the VehLds image, padded to 16 bytes
    std::vector<int32_t> tasks;       // [2][cars_per_block * tasks_per_car][4] the sweep's task tables (DeviceParams::task_tab)
    std::vector<int32_t> tasks_win;   // [cars_per_block * win_tasks_per_car][4] the window-only table, behind them in the parameter image (plan_window_table)
    std::vector<int32_t> wg;          // [n_wg][4] the workgroup table: block offset (set by layout_images), first car, cars, track.  Uploaded for several tracks only
    std::vector<int32_t> env_track;   // [n_envs]; uploaded for several tracks only
    int n_wg = 0;                     // workgroups of a step launch
};

// workgroup shape: whole envs, at most 16 cars (K1 / K3 run on the lanes of one wave), two workgroups per CU
// (<= 80 KiB of LDS each) so that 8 waves per SIMD hide the latency of the field loads
int plan_shape(DeviceParams& P, const Switches& sw)
{
    const int unit = P.cars_per_env;
    const int wpb = sw.waves_per_block, lds_cap = sw.lds_cap;
    int want = (FTGP_MAX_CARS_PER_BLOCK / unit) * unit;
    // small batches: fewer cars per workgroup so that every CU gets work.  Up to four envs per CU a batch runs best as ONE workgroup per CU
    // (its step is the driver -> dynamics latency chain plus one sweep task per wave: a second workgroup on the CU only competes for issue
    // slots -- 1024 envs: 9.1 us per step with 256 workgroups of 4, 9.8 with 512 of 2; 512 envs: 8.8 / 9.0); larger batches take two
    // workgroups per CU (1536 envs: 10.7 us with 512 workgroups of 3, 13.9 with 256 of 6) -- profiles/round5/config2_shapes.log
    const int n_units = P.n_cars / unit;
    const int n_cu = P.n_cu > 0 ? P.n_cu : 256;
    const int per_cu = (n_units + n_cu - 1) / n_cu;
    const int spread = (per_cu <= 4 ? std::max(1, per_cu) : std::max(1, n_units / (2 * n_cu))) * unit;
    int cpb = std::min(want, spread);
    if (sw.cars_per_block >= unit && sw.cars_per_block <= FTGP_MAX_CARS_PER_BLOCK) cpb = (sw.cars_per_block / unit) * unit;
    while (cpb > unit && lds_layout(P, cpb, wpb) > lds_cap) cpb -= unit;
    if (lds_layout(P, cpb, wpb) > 160 * 1024) {
        snprintf(g_err, sizeof g_err, "one env of %d car(s) with a %d-ray scan does not fit the 160 KiB LDS", unit, P.n_rays);
        return FTGP_ERR_ARG;
    }
    if (sw.verbose)
        fprintf(stderr, "ftgp_create: %d cars x %d waves per workgroup, %d B of LDS (cap %d)\n", cpb, wpb, lds_layout(P, cpb, wpb), lds_cap);
    return 0;
}

// the fan: binary32 ray table (zero-padded to 16 bytes) and binary64 directions
void plan_fan(const FtgpConfig& cfg, std::vector<float>& ray, std::vector<double>& fan)
{
    const int R = cfg.n_rays;
    ray.assign((size_t)pad16(sizeof(float) * 2 * (size_t)R) / sizeof(float), 0.0f);
    fan.assign(2 * (size_t)R, 0.0);
    for (int j = 0; j < R; ++j) {
        // mushr.em.xml:112-117: phi_j = radians(360/R*j - 90); the ray (+z of the site) is (sin phi, -cos phi, 0)
        const double phi = ((360.0 / (double)R) * (double)j - 90.0) * (M_PI / 180.0);
        fan[2 * (size_t)j] = cfg.fan_dirs ? cfg.fan_dirs[2 * (size_t)j] : sin(phi);
        fan[2 * (size_t)j + 1] = cfg.fan_dirs ? cfg.fan_dirs[2 * (size_t)j + 1] : -cos(phi);
        ray[2 * (size_t)j] = (float)fan[2 * (size_t)j]; ray[2 * (size_t)j + 1] = (float)fan[2 * (size_t)j + 1];
        // The rangefinders' own fan is point-symmetric: site j + n/2 looks exactly opposite to site j.  The BINARY32 table says so to the last
        // bit (its second half is the negated first half -- the roundings of libm's sin / cos of phi + pi need not be), which is what lets the
        // sweep derive a ray from its opposite; a caller's fan_dirs is taken as it comes.  The binary64 fan of FAKELIDAR mode is libm's value
        // for every site, as include/ftgp.h says for fan_dirs == NULL (round 4 negated it too: a last-bit difference from the documented fan).
        if (!cfg.fan_dirs && R % 2 == 0 && j >= R / 2) {
            ray[2 * (size_t)j] = -ray[2 * (size_t)(j - R / 2)]; ray[2 * (size_t)j + 1] = -ray[2 * (size_t)(j - R / 2) + 1];
        }
    }
}

// a task may be a pair of opposite ray groups: the binary32 fan is point-symmetric to the bit (ray j + n/2 is the negated ray j), FTGP_NO_PAIRS unset
bool fan_allows_pairs(const std::vector<float>& ray, int R, const Switches& sw)
{
    const int halfR = R / 2;
    bool sym = R % 2 == 0 && !sw.no_pairs;
    for (int j = 0; sym && j < halfR; ++j)
        sym = ray[2 * (size_t)(j + halfR)] == -ray[2 * (size_t)j] && ray[2 * (size_t)(j + halfR) + 1] == -ray[2 * (size_t)j + 1] &&
              std::signbit(ray[2 * (size_t)(j + halfR)]) != std::signbit(ray[2 * (size_t)j]) && std::signbit(ray[2 * (size_t)(j + halfR) + 1]) != std::signbit(ray[2 * (size_t)j + 1]);
    return sym;
}

// the sweep's work list (lidar_groups): draw g -> (kidx = g / cars_per_block, car slot = g % cars_per_block), task = group_order[kidx]
void plan_task_order(const FtgpConfig& cfg, const std::vector<float>& ray, const Switches& sw, DeviceParams& P)
{
    const int R = cfg.n_rays, halfR = R / 2;
    const bool sym = fan_allows_pairs(ray, R, sw);
    std::vector<int> tasks;
    if (!sym) for (int j0 = 0; j0 < R; j0 += FTGP_WAVE) tasks.push_back(j0);
    else {
        int j0 = 0;
        for (; j0 + FTGP_WAVE <= halfR; j0 += FTGP_WAVE) tasks.push_back(j0 | (1 << 16));
        if (j0 < halfR) tasks.push_back(j0 | ((halfR - j0 <= FTGP_WAVE / 2 ? 2 : 1) << 16));
    }
    // expected march length of a task ~ how far its rays look along the car's axis: |cos| of the angle between the group's middle ray
    // and the axis (ray 0 looks backwards, ray n/2 ahead); ties keep index order
    std::vector<std::pair<double, int>> key;
    for (int t : tasks) {
        const double mid = std::min((double)R - 1.0, (double)(t & 0xffff) + 31.5);
        key.push_back({ sw.group_order_plain ? 0.0 : -fabs(cos(2.0 * M_PI * mid / (double)R)), t });
    }
    std::stable_sort(key.begin(), key.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
    // the cheapest pairs -- the last tasks a sweep draws -- go out as two single groups each: the waves then end a sweep within ONE short
    // group of each other, not within two (the set-up shared inside a pair is worth less than that at the very end)
    const int tail = sw.pair_tail;
    std::vector<int> order;
    for (size_t k = 0; k < key.size(); ++k) {
        const int t = key[k].second;
        if ((t >> 16) == 1 && (int)(key.size() - k) <= tail) { order.push_back(t & 0xffff); order.push_back((t & 0xffff) + halfR); }
        else order.push_back(t);
    }
    P.tasks_per_car = (int)order.size();
    for (size_t k = 0; k < order.size(); ++k) P.group_order[k] = order[k];
    // mate_masks(): a ray of a group lies within 32 spacings of the rangefinders' uniform fan of the group's middle ray; + 1.2 degrees for the
    // slack in the rays' own test (acos 0.9999 = 0.81 degrees) and rounding.  A caller's fan has no such bound: every mate is looked at.
    const double gamma = 32.0 * (2.0 * M_PI / (double)R) + 0.021;
    if (cfg.fan_dirs || gamma >= 1.5) { P.group_cg = -2.0f; P.group_sg = 0.0f; }
    else { P.group_cg = (float)cos(gamma); P.group_sg = (float)sin(gamma); }
    if (sw.verbose) fprintf(stderr, "ftgp_create: %d sweep tasks per car (%s)\n", P.tasks_per_car, sym ? "pairs of opposite ray groups" : "single groups");
}

// the sweep's task tables (DeviceParams::task_tab): draw g is task g / cars_per_block of car slot g % cars_per_block, with everything the
// draw and the delivery need precomputed
int plan_task_table(const DeviceParams& P, std::vector<int32_t>& tt)
{
    const int cpb = P.cars_per_block, ntasks = cpb * P.tasks_per_car, R = P.n_rays, halfR = R / 2;
    if (P.tasks_per_car > 256 || R > 0x4000) return fail(FTGP_ERR_ARG, "internal: the task table's fields are too narrow for this fan%s");
    tt.assign(2 * 4 * (size_t)ntasks, 0);
    auto wclass = [&](int first, int lim) {          // rays first .. min(first + 63, lim - 1) against the window [eighth, R - eighth)
        const int last = std::min(first + FTGP_WAVE, lim) - 1, lo = P.eighth, hi = R - P.eighth;
        if (last < lo || first >= hi || lo >= hi) return 0;
        return (first >= lo && last < hi) ? 1 : 2;
    };
    for (int g = 0; g < ntasks; ++g) {
        const int kidx = g / cpb, c = g % cpb, ent = P.group_order[kidx], j0 = ent & 0xffff, kind = ent >> 16;
        const int w0 = kind == 2 ? 2 : wclass(j0, kind == 1 ? halfR : R), w1 = kind == 1 ? wclass(j0 + halfR, R) : 0;
        const uint32_t plain = (uint32_t)j0 | (uint32_t)kind << 14 | (uint32_t)c << 16;
        int32_t* a = &tt[4 * (size_t)g];
        int32_t* b = &tt[4 * (size_t)(ntasks + g)];
        a[0] = (int32_t)(plain | (uint32_t)w0 << 20 | (uint32_t)w1 << 22 | (uint32_t)(j0 == 0 ? 1 : 0) << 24);
        b[0] = (int32_t)plain;
        a[1] = b[1] = c * (int)sizeof(LidarFrame) | kidx << 16;
        a[2] = b[2] = c * P.ranges_stride * 4;
        a[3] = b[3] = 4 * (c * P.win_floats + (P.eighth & 3) - P.eighth);
    }
    return 0;
}

// The window-only table (DeviceParams::task_tab's third; tt: the two tables of plan_task_table).  Inside a launch whose drivers read the scan, a range
// of any step but the last has one reader, the next step's driver, and that reads ranges[0] and ranges[eighth : n - eighth]: every other ray of
// such a step -- the rear quarter of the fan, where the rays look down the track and march longest -- is overwritten unread.  So those steps draw
// from a list of their own, cut from the live rays alone (ftgp_window_cut.h): pairs over the sideways zone, single groups over the forward cone,
// and what is left of both, with ray 0, in GATHER tasks (kind 3) whose lanes take their rays from a few runs -- 13 full marches per car at 1080
// rays where the first table's tasks, less their dead rays, took 15.  The list has its own order (win_group_order, the first table's key: |cos|
// of the task's middle ray, for a gather the mean |cos| over its rays; FTGP_PAIR_TAIL splits its cheapest pairs) and its own ranks ([1]), so
// mate_masks() is run on win_group_order for a step that draws from it.  Behind the draws, [gathers][4]: the runs of each gather task
// (ftgp_device.h).  mmask_stride and group_order's size are the first table's, so the list never has more tasks than that: the tail's splits
// give way first, and a list still longer (FTGP_PAIR_TAIL=0 at a few fan sizes) is dropped for the first table, as a fan without an unread
// ray (n_rays < 8) gets it.  FTGP_SCAN_EVERY_STEP: no such table, win_tasks_per_car = 0.
void plan_window_table(const Switches& sw, const std::vector<float>& ray, const std::vector<int32_t>& tt, DeviceParams& P, std::vector<int32_t>& tw)
{
    const int cpb = P.cars_per_block, R = P.n_rays, halfR = R / 2;
    tw.clear();
    P.win_tasks_per_car = 0;
    for (int k = 0; k < FTGP_MAX_GROUPS; ++k) P.win_group_order[k] = 0;
    if (sw.scan_every_step) {
        if (sw.verbose) fprintf(stderr, "ftgp_create: FTGP_SCAN_EVERY_STEP: every step of a launch sweeps and stores every ray\n");
        return;
    }
    const bool dead = P.eighth > 0;                  // some ray but ray 0 lies outside [eighth, R - eighth)
    const FtgpWindowCut cut = ftgp_window_cut(R, P.eighth, fan_allows_pairs(ray, R, sw));
    // longest first: |cos| of the angle between the car's axis and the task's middle ray; a gather: the mean over its rays
    auto along = [&](double j) { return fabs(cos(2.0 * M_PI * j / (double)R)); };
    struct Ent { double key; int ent, gather; };
    std::vector<Ent> key;
    for (int j0 : cut.pairs) key.push_back({ -along(j0 + 31.5), j0 | 1 << 16, -1 });
    for (int j0 : cut.singles) key.push_back({ -along(j0 + 31.5), j0, -1 });
    for (size_t q = 0; q < cut.gathers.size(); ++q) {
        double sum = 0.0; int lanes = 0;
        for (const FtgpWindowCut::Run& r : cut.gathers[q]) { for (int j = r.first; j < r.first + r.second; ++j) sum += along(j); lanes += r.second; }
        key.push_back({ -sum / lanes, lanes | (int)q << 7 | 3 << 16, (int)q });
    }
    if (sw.group_order_plain) for (Ent& k : key) k.key = 0.0;
    std::stable_sort(key.begin(), key.end(), [](const Ent& a, const Ent& b) { return a.key < b.key; });
    std::vector<int> order;
    for (int tail = std::max(0, sw.pair_tail); ; --tail) {
        order.clear();
        for (size_t k = 0; k < key.size(); ++k) {
            const int t = key[k].ent;
            if ((t >> 16) == 1 && (int)(key.size() - k) <= tail) { order.push_back(t & 0xffff); order.push_back((t & 0xffff) + halfR); }
            else order.push_back(t);
        }
        if ((int)order.size() <= P.tasks_per_car || tail == 0) break;
    }
    if (!dead || (int)order.size() > P.tasks_per_car || cut.gathers.size() > 127) {        // the first table again
        P.win_tasks_per_car = P.tasks_per_car;
        for (int k = 0; k < P.tasks_per_car; ++k) P.win_group_order[k] = P.group_order[k];
        tw.assign(tt.begin(), tt.begin() + 4 * (size_t)cpb * P.tasks_per_car);
        for (size_t g = 0; g < (size_t)cpb * P.tasks_per_car; ++g) tw[4 * g] |= FTGP_TASK_MASKED;      // partial groups, every window class: no plain draw
        if (sw.verbose) fprintf(stderr, "ftgp_create: %d of them on the window-only steps of a launch\n", P.win_tasks_per_car);
        return;
    }
    P.win_tasks_per_car = (int)order.size();
    for (size_t k = 0; k < order.size(); ++k) P.win_group_order[k] = order[k];
    const int ntasks = cpb * P.win_tasks_per_car;
    tw.assign(4 * ((size_t)ntasks + cut.gathers.size()), 0);
    for (int g = 0; g < ntasks; ++g) {
        const int kidx = g / cpb, c = g % cpb, ent = order[(size_t)kidx], kind = ent >> 16;
        const int32_t* a = &tt[4 * (size_t)c];           // the car slot's offsets: any draw of the first table has them
        int32_t* w = &tw[4 * (size_t)g];
        bool zero = false;
        if (kind == 3) for (const FtgpWindowCut::Run& r : cut.gathers[(size_t)((ent >> 7) & 127)]) zero = zero || r.first == 0;
        // every ray of a pair or a single group lies in the window (class 1); a gather tests per ray (class 2: ray 0 goes to its own float).
        // A pair or a single group is a PLAIN draw -- 64 live rays a group, no ray 0 (ftgp_window_cut.h) --, a gather is not (FTGP_TASK_MASKED).
        w[0] = (int32_t)((uint32_t)(ent & 0x3fff) | (uint32_t)kind << 14 | (uint32_t)c << 16 | (kind == 3 ? 2u : 1u) << 20 | (kind == 1 ? 1u : 0u) << 22 | (zero ? 1u : 0u) << 24 |
                           (kind == 3 ? (uint32_t)FTGP_TASK_MASKED : 0u));
        w[1] = (a[1] & 0xffff) | kidx << 16; w[2] = a[2]; w[3] = a[3];
    }
    for (size_t q = 0; q < cut.gathers.size(); ++q) {   // a gather's runs: (first ray - first lane) & 0xffff | first lane << 16; a run it does not have starts at lane 64
        int32_t* w = &tw[4 * ((size_t)ntasks + q)];
        int lane = 0;
        for (size_t k = 0; k < 4; ++k) {
            if (k < cut.gathers[q].size()) { w[k] = (int32_t)((uint32_t)((cut.gathers[q][k].first - lane) & 0xffff) | (uint32_t)lane << 16); lane += cut.gathers[q][k].second; }
            else w[k] = (int32_t)(64u << 16);
        }
    }
    if (sw.verbose) fprintf(stderr, "ftgp_create: %d of them on the window-only steps of a launch\n", P.win_tasks_per_car);
}

// the map's diagonal in world units: no ray between two cars on the map is longer
double track_diagonal(const FtgpTrack& t) { return hypot((double)t.width * t.px_size_x, (double)t.height * t.px_size_y); }

// the VehLds image: the vehicle constants as the step kernel stages them into LDS; diag = the longest map diagonal of the handle's tracks
void plan_vehicle(const DeviceParams& P, double diag, const Switches& sw, std::vector<unsigned char>& img)
{
    const FtgpVehicle& v = P.veh;
    img.assign((size_t)pad16(sizeof(VehLds)), 0);
    VehLds vl; memset(&vl, 0, sizeof vl);
    vl.v = P.veh; for (int i = 0; i < 4; ++i) vl.wheel_load[i] = P.wheel_load[i];
    // every part of a car that a ray can see (chassis box, LiDAR puck) lies within rmax of the car's origin; 10 % margin
    const double cx = std::max(fabs(v.box_xmin), fabs(v.box_xmax)), cy = std::max(fabs(v.box_ymin), fabs(v.box_ymax));
    const double rmax = std::max(sqrt(cx * cx + cy * cy), sqrt(v.lidar_x * v.lidar_x + v.lidar_y * v.lidar_y) + v.lidar_ring_radius);
    vl.cull_radius = (float)(1.1 * rmax);
    {   // The sweep leaves the puck's circle out when the box's time is the minimum of the two to the bit: the puck inside the box with `need` to spare on
        // every side.  Both tests work on the same binary32 origin and direction in the mate's frame, so only what follows them counts, and far away that
        // is the cancellation in the circle's discriminant disc = bq^2 - cq: bq^2 and cq are both about D^2 at D units, their difference is at most r0^2.
        // What enters disc: two roundings of bq (times 2 bq), three of cq, and the direction's norm, which the formula takes for 1 (disc is off by
        // (|d|^2 - 1) cq).  With an error of e in disc the circle is met as if its radius were sqrt(r0^2 + e) <= r0 + e / (2 r0), up to that much EARLIER than
        // the true puck.  e = 5 * 2^-24 * D^2: the largest seen is 3.9 (190 000 hits at 40 to 55 units, oracle with and without the circle:
        // tests/test_crowded_envs.py repeats the measurement); adding up every rounding's worst case would give about 8, which no ray gets near.
        // D = the longest ray between two cars on the map: the diagonal of the handle's largest track.  40 x 40 units, r0 = 0.03: 0.0159
        // (MuSHR has 0.0161 on its tightest side, the tricycle 0.0175: both keep the short path; on a larger map they take the circle test).
        const double r = v.lidar_ring_radius;
        const double need = r > 0.0 ? 5.0 * ldexp(1.0, -24) * diag * diag / (2.0 * r) : 0.0;
        const double have = std::min(std::min(v.lidar_x - r - v.box_xmin, v.box_xmax - (v.lidar_x + r)), std::min(v.lidar_y - r - v.box_ymin, v.box_ymax - (v.lidar_y + r)));
        vl.puck_in_box = (have >= need && !sw.puck_test) ? 1 : 0;
        if (sw.verbose)
            fprintf(stderr, "ftgp_create: inter-vehicle rays test %s (the puck lies %.4f inside the box, %.4f needed on a map of diagonal %.2f)\n",
                    vl.puck_in_box ? "the box only" : "the box and the puck's circle", have, need, diag);
    }
    vl.box_xmin_f = (float)v.box_xmin; vl.box_xmax_f = (float)v.box_xmax; vl.box_ymin_f = (float)v.box_ymin; vl.box_ymax_f = (float)v.box_ymax;
    vl.lidar_x_f = (float)v.lidar_x; vl.lidar_y_f = (float)v.lidar_y; vl.ring_radius_f = (float)v.lidar_ring_radius;
    memcpy(img.data(), &vl, sizeof vl);
}

// What of the parameter block depends on the track: image size and strides, sector planes, pixel geometry, the wall-contact reach, the
// march's snap distance, the frame's edge margin.  P.n_sectors (chosen for the whole batch) must be set.
void plan_track_params(const FtgpConfig& cfg, const FtgpTrack& t, DeviceParams& P)
{
    const FtgpVehicle& v = cfg.vehicle;
    P.width = t.width; P.height = t.height; P.words_per_row = t.words_per_row; P.fstride = t.width + 2;
    P.plane256 = ftgp_plane256(t.width, t.height);
    // a ray's sector is always found among all FTGP_SECTORS; the table says which plane serves it
    P.n_planes = ftgp_sector_table(P.sector_tab, P.n_sectors, t.width + 2, P.plane256);
    P.px_size_x = t.px_size_x; P.px_size_y = t.px_size_y; P.origin_x = t.origin_x; P.origin_y = t.origin_y;
    P.inv_px_x = 1.0 / t.px_size_x; P.inv_px_y = 1.0 / t.px_size_y;
    P.inv_px_x_f = (float)P.inv_px_x; P.inv_px_y_f = (float)P.inv_px_y;
    {   // chessboard reach of the largest wall-contact window
        const double rmax = std::max(v.contact_radius, cfg.bubble_wrap ? v.softener_radius : 0.0);
        P.contact_reach = std::max((int)ceil(rmax * P.inv_px_x), (int)ceil(rmax * P.inv_px_y));
    }
    P.snap_eps = ftgp_snap_eps(t.width, t.height);
    P.edge_margin = (float)(v.lidar_ring_radius * std::max(P.inv_px_x, P.inv_px_y) * 1.001 + 2.0);
}

// the track's bitmaps and run lengths, and its spawn table
void plan_track_tables(const FtgpTrack& t, const DeviceParams& P, HostTables& tab, std::vector<double>& spawn)
{
    build_tables(t, P.contact_reach, tab);
    spawn.assign(4 * FTGP_PATH_POINTS, 0.0);
    ftgp_spawn_table(t, spawn.data());
}

// Workgroup order of a multi-track launch (FTGP_TRACK_ORDER=blocks|xcd).  Workgroups are dealt round robin over the 8 XCDs, so workgroups b
// and b + 8 share an L2 (observed, not promised).  blocks: the workgroups in car order, track after track -- every XCD then holds a share
// of every track's field.  xcd: the k-th workgroup in car order takes the k-th index of the grid sorted by (b % 8, b), so that each track
// owns a run of residues b % 8, in proportion to its number of workgroups, and an L2 holds the fields of one or two tracks.  Results do
// not depend on the order.
// The workgroup table: whole envs of one track per workgroup, each block of envs its own workgroups with a ragged last one.  wg[4 b ..]
// = (0: the block offset, filled in by layout_images; first car; cars; track).
void plan_workgroups(int cpb, int cpe, const int32_t* envs_per_track, int n_tracks, int order, std::vector<int32_t>& wg)
{
    std::vector<int32_t> list;
    int first = 0;
    for (int t = 0; t < n_tracks; ++t) {
        const int end = first + envs_per_track[t] * cpe;
        for (int c0 = first; c0 < end; c0 += cpb) { const int32_t e[4] = { 0, c0, std::min(cpb, end - c0), t }; list.insert(list.end(), e, e + 4); }
        first = end;
    }
    const int n = (int)list.size() / 4;
    std::vector<int> slot(n);
    for (int k = 0; k < n; ++k) slot[k] = k;
    if (order == kOrderXcd) {
        int k = 0;
        for (int r = 0; r < 8; ++r)
            for (int b = r; b < n; b += 8) slot[k++] = b;
    }
    wg.assign(list.size(), 0);
    for (int k = 0; k < n; ++k) std::copy(&list[4 * (size_t)k], &list[4 * (size_t)k] + 4, &wg[4 * (size_t)slot[k]]);
}

// ftgp_create / ftgp_create_tracks, step 2: the plan of the batch (shape, sectors, fan, tasks: as for one track of all n_envs envs), then
// every track's own block, tables and spawn table, and the workgroup table.  A function of its arguments; host arithmetic only.
// envs_per_track: [n_tracks], summing to cfg.n_envs (cfg.track is not read).  n_cu: compute units of the device (the workgroup shape
// depends on it).
int plan(const FtgpConfig& cfg, const FtgpTrack* tracks, const int32_t* envs_per_track, int n_tracks, int n_cu, const Switches& sw, Plan& pl)
{
    const FtgpVehicle& v = cfg.vehicle;
    pl.tracks.assign((size_t)n_tracks, Plan::Track());
    DeviceParams& P = pl.tracks[0].P;               // the batch's values first; the tracks' own follow below
    P.n_envs = cfg.n_envs; P.cars_per_env = cfg.cars_per_env; P.n_cars = cfg.n_envs * cfg.cars_per_env;
    P.n_rays = cfg.n_rays; P.lap_target = cfg.lap_target; P.spawn_mode = cfg.spawn_mode; P.env_base = cfg.env_base;
    P.ranges_stride = (cfg.n_rays + 31) & ~31;      // rows start on 128-B boundaries
    P.seed = cfg.seed; P.dt = cfg.dt;
    P.rpp = (2 * M_PI) / (double)cfg.n_rays;
    P.two_over_rpp = (float)(2.0 / P.rpp);
    P.bubble_wrap = cfg.bubble_wrap ? 1 : 0;        // cfg.naive_flatten: accepted, no effect on a planar model (custom.py:1338-1339)
    P.lidar_mode = cfg.lidar_mode;
    P.map_size = cfg.map_size > 0.0 ? cfg.map_size : 40.0;                     // 20 * scale, custom.py:1155,1382
    P.n_sectors = sector_count(cfg, sw); P.slice_factor = FTGP_SLICE_FACTOR(FTGP_SLOPE_SLICES);
    P.veh = cfg.vehicle;
    {   // static wheel loads from the wheelbase split
        const double wtot = v.mass * v.gravity;
        if (v.kind == FTGP_VEHICLE_TRICYCLE) {       // two driven wheels behind the origin, the caster (wheel 2) in front
            const double a_f = v.wheel_x[2], a_r = -0.5 * (v.wheel_x[0] + v.wheel_x[1]);
            P.wheel_load[0] = P.wheel_load[1] = 0.5 * (wtot * (a_f / (a_f + a_r)));
            P.wheel_load[2] = wtot * (a_r / (a_f + a_r)); P.wheel_load[3] = 0.0;
        } else {
            const double a_f = 0.5 * (v.wheel_x[0] + v.wheel_x[1]), a_r = -0.5 * (v.wheel_x[2] + v.wheel_x[3]);
            P.wheel_load[0] = P.wheel_load[1] = 0.5 * (wtot * (a_r / (a_f + a_r)));
            P.wheel_load[2] = P.wheel_load[3] = 0.5 * (wtot * (a_f / (a_f + a_r)));
        }
    }
    P.eighth = (int)((double)cfg.n_rays / 8.0);                    // nidc.py:18
    // the largest cover count any positive sample can produce (that of the smallest positive float), over both drivers
    const double tiny = (double)1.401298464e-45f;
    P.cover_kmax = std::max(1, std::max(cover_count_host(0.24, P.rpp, tiny), cover_count_host(0.12, P.rpp, tiny)));
    P.win_floats = ((P.eighth & 3) + (cfg.n_rays - 2 * P.eighth) + 1 + 3) & ~3;       // window at float (eighth % 4), ranges[0] in the last float
    P.n_cu = n_cu;
    if ((cfg.n_rays + FTGP_WAVE - 1) / FTGP_WAVE > FTGP_MAX_GROUPS) return fail(FTGP_ERR_ARG, "n_rays above 16384 is not supported%s");
    if (int rc = plan_shape(P, sw)) return rc;
    plan_fan(cfg, pl.ray, pl.fan);
    plan_task_order(cfg, pl.ray, sw, P);
    if (int rc = plan_task_table(P, pl.tasks)) return rc;
    plan_window_table(sw, pl.ray, pl.tasks, P, pl.tasks_win);
    {   // cover-count thresholds: nidc (car_width 0.12, nidc.py:5) then fast (0.06, fast.py:4), each padded to the staged size
        const size_t stride = (size_t)P.cover_kmax + 1, padded = (size_t)pad16(sizeof(float) * stride) / sizeof(float);
        pl.cover.assign(stride + padded + 4, 0.0f);
        build_cover_table(0.12, cfg.n_rays, P.cover_kmax, pl.cover.data());
        build_cover_table(0.06, cfg.n_rays, P.cover_kmax, pl.cover.data() + stride);
    }
    double diag = 0.0;                              // of the largest track
    pl.env_track.clear();
    for (int t = 0; t < n_tracks; ++t) {
        Plan::Track& k = pl.tracks[(size_t)t];
        k.P = P;
        plan_track_params(cfg, tracks[t], k.P);
        plan_track_tables(tracks[t], k.P, k.tab, k.spawn);
        k.clear.assign(2 * FTGP_PATH_POINTS, 0.0);
        ftgp_start_table(tracks[t], k.spawn.data(), k.clear.data());
        k.path.assign(tracks[t].path, tracks[t].path + 2 * FTGP_PATH_POINTS);
        diag = std::max(diag, track_diagonal(tracks[t]));
        pl.env_track.insert(pl.env_track.end(), (size_t)envs_per_track[t], t);
    }
    plan_vehicle(P, diag, sw, pl.veh);
    plan_workgroups(P.cars_per_block, cfg.cars_per_env, envs_per_track, n_tracks, sw.track_order, pl.wg);
    pl.n_wg = (int)pl.wg.size() / 4;
    if (sw.verbose)
        fprintf(stderr, "ftgp_create: %d track(s), %d workgroups in %s order\n", n_tracks, pl.n_wg, sw.track_order == kOrderXcd ? "xcd" : "blocks");
    return 0;
}

// The device addresses that the parameter blocks and the staging images point to: the upload's allocations (the host checks make them up).
struct DeviceAddrs {
    struct Track { const uint16_t* field; const double* edt; const uint32_t* bits, * nearbits; };
    std::vector<Track> trk;
    const double* fan = nullptr, * path = nullptr, * spawn = nullptr;      // path, spawn: every track's, track after track
    const void* veh = nullptr; const float* ray = nullptr, * cover = nullptr;
    CarState* cars = nullptr; float* ranges = nullptr; int64_t* steps = nullptr;
    double* wg_metrics = nullptr; unsigned int* wg_ticket = nullptr; double* metrics_dev = nullptr, * metrics_host = nullptr;     // null: no fused metrics
    double* wg_metrics_host = nullptr;
    const unsigned char* params = nullptr, * stage = nullptr;              // where the two images will lie
};

// Sizes of the two images.  Parameter image: track 0's block | (several tracks: the workgroup table) | the sweep's task tables, all three | the
// blocks of tracks 1 .. T - 1.  Staging image, one per track: the LDS bytes [off_params, off_cars) as every workgroup of the track wants
// them, then both drivers' cover tables.
struct ImageSizes { size_t head, wg, tasks, params, stage_head, stage; };
ImageSizes image_sizes(const Plan& pl)
{
    const size_t T = pl.tracks.size();
    const DeviceParams& P = pl.tracks[0].P;
    ImageSizes z;
    z.head = FTGP_PARAMS_BYTES; z.wg = T > 1 ? sizeof(int32_t) * pl.wg.size() : 0; z.tasks = sizeof(int32_t) * (pl.tasks.size() + pl.tasks_win.size());
    z.params = z.head + z.wg + z.tasks + (T - 1) * z.head + 16;
    z.stage_head = (size_t)(P.off_cars - P.off_params);
    z.stage = z.stage_head + 2 * (size_t)P.stage_cover;
    return z;
}

struct Images {
    std::vector<unsigned char> params, stage;
    std::vector<size_t> blocks;       // byte offset of each track's parameter block in the parameter image (track 0: 0)
    DeviceParams P0;                  // track 0's finished block
};

// ftgp_create, between plan and upload: both images as they go to the device, every pointer set.  Host arithmetic only (no HIP call).
void layout_images(const Plan& pl, const DeviceAddrs& a, Images& im)
{
    const DeviceParams& P = pl.tracks[0].P;         // (the LDS layout is the batch's)
    const int T = (int)pl.tracks.size();
    const ImageSizes z = image_sizes(pl);
    const size_t sz_path = sizeof(double) * 2 * FTGP_PATH_POINTS, stride = (size_t)P.cover_kmax + 1;
    im.blocks.assign((size_t)T, 0);
    for (int k = 1; k < T; ++k) im.blocks[(size_t)k] = z.head + z.wg + z.tasks + (size_t)(k - 1) * z.head;
    im.params.assign(z.params, 0);
    im.stage.assign(z.stage * T, 0);
    for (int k = 0; k < T; ++k) {
        DeviceParams Q = pl.tracks[(size_t)k].P;     // (a copy as it lies, padding included)
        const DeviceAddrs::Track& b = a.trk[(size_t)k];
        Q.edt = b.edt; Q.fan_dirs = a.fan; Q.field = b.field;
        Q.wg_metrics = a.wg_metrics; Q.wg_ticket = a.wg_ticket; Q.metrics_dev = a.metrics_dev; Q.metrics_host = a.metrics_host;
        Q.wg_metrics_host = a.wg_metrics_host;
        Q.bits = b.bits; Q.nearbits = b.nearbits; Q.path = a.path + 2 * FTGP_PATH_POINTS * (size_t)k; Q.spawn = a.spawn + 4 * FTGP_PATH_POINTS * (size_t)k;
        Q.veh_dev = a.veh;
        Q.ray_dir = a.ray; Q.cover_thr = a.cover; Q.cars = a.cars; Q.ranges = a.ranges; Q.steps = a.steps;
        unsigned char* s = im.stage.data() + z.stage * k;
        memcpy(s, &Q, offsetof(DeviceParams, veh));      // every pointer of the head is set by now
        memcpy(s + (P.off_veh - P.off_params), pl.veh.data(), pl.veh.size());
        memcpy(s + (P.off_path - P.off_params), pl.tracks[(size_t)k].path.data(), sz_path);
        memcpy(s + (P.off_ray - P.off_params), pl.ray.data(), sizeof(float) * pl.ray.size());
        memcpy(s + z.stage_head, pl.cover.data(), sizeof(float) * stride);
        memcpy(s + z.stage_head + P.stage_cover, pl.cover.data() + stride, sizeof(float) * stride);
        Q.stage_img = a.stage + z.stage * k;
        Q.task_tab = reinterpret_cast<const int32_t*>(a.params + z.head + z.wg);
        memcpy(im.params.data() + im.blocks[(size_t)k], &Q, sizeof(DeviceParams));
        if (k == 0) memcpy(&im.P0, &Q, sizeof Q);
    }
    if (T > 1) {     // the workgroup table: each entry's block offset
        std::vector<int32_t> wg = pl.wg;
        for (size_t b = 0; b < wg.size(); b += 4) wg[b] = (int32_t)im.blocks[(size_t)wg[b + 3]];
        memcpy(im.params.data() + z.head, wg.data(), z.wg);
    }
    memcpy(im.params.data() + z.head + z.wg, pl.tasks.data(), sizeof(int32_t) * pl.tasks.size());
    memcpy(im.params.data() + z.head + z.wg + sizeof(int32_t) * pl.tasks.size(), pl.tasks_win.data(), sizeof(int32_t) * pl.tasks_win.size());
}

// nidc or fast, for every car or for some car of the roster
bool uses_disparity_driver(const FtgpEnv* e, int policy)
{
    if (policy == FTGP_POLICY_NIDC || policy == FTGP_POLICY_FAST) return true;
    if (policy != FTGP_POLICY_PER_CAR) return false;
    for (int k = 0; k < e->P.cars_per_env; ++k) if (e->P.car_policy[k] == FTGP_POLICY_NIDC || e->P.car_policy[k] == FTGP_POLICY_FAST) return true;
    return false;
}

// what the device drivers nidc and fast need of the scan
int check_disparity_shape(const DeviceParams& P)
{
    if (P.n_rays < 8) return fail(FTGP_ERR_ARG, "nidc/fast need n_rays >= 8 (they drop len/8 rays from each end)%s");
    if (P.n_rays - 2 * P.eighth > FTGP_WAVE * FTGP_WAVE) return fail(FTGP_ERR_ARG, "the device drivers handle at most 4096 samples in the front window%s");
    return 0;
}

// The six instantiations of ftgp_step_kernel<MULTI, FAKE, ROSTER, false>, and the six of multi-track handles (TRACKS = true).  FAKELIDAR
// always runs the roster one.  The one-track names keep their three flags: what ftgp_kernel_name has always returned.
struct StepKernel { void (*fn)(const DeviceParams*, int, int, int); const char* name; };
const StepKernel kStepKernels[2][2][3] = {      // [multi-track][multi][0: single driver, 1: roster, 2: FAKELIDAR]
  { { { ftgp_step_kernel<false, false, false, false>, "ftgp_step_kernel<false, false, false>" },
      { ftgp_step_kernel<false, false, true, false>, "ftgp_step_kernel<false, false, true>" },
      { ftgp_step_kernel<false, true, true, false>, "ftgp_step_kernel<false, true, true>" } },
    { { ftgp_step_kernel<true, false, false, false>, "ftgp_step_kernel<true, false, false>" },
      { ftgp_step_kernel<true, false, true, false>, "ftgp_step_kernel<true, false, true>" },
      { ftgp_step_kernel<true, true, true, false>, "ftgp_step_kernel<true, true, true>" } } },
  { { { ftgp_step_kernel<false, false, false, true>, "ftgp_step_kernel<false, false, false, true>" },
      { ftgp_step_kernel<false, false, true, true>, "ftgp_step_kernel<false, false, true, true>" },
      { ftgp_step_kernel<false, true, true, true>, "ftgp_step_kernel<false, true, true, true>" } },
    { { ftgp_step_kernel<true, false, false, true>, "ftgp_step_kernel<true, false, false, true>" },
      { ftgp_step_kernel<true, false, true, true>, "ftgp_step_kernel<true, false, true, true>" },
      { ftgp_step_kernel<true, true, true, true>, "ftgp_step_kernel<true, true, true, true>" } } },
};

// ftgp_step_kernel<MULTI, false, ROSTER, TRACKS, true>: launches with the table of per-car dynamics on (ftgp_set_dynamics)
const StepKernel kStepKernelsDyn[2][2][2] = {   // [multi-track][multi][roster]
  { { { ftgp_step_kernel<false, false, false, false, true>, "ftgp_step_kernel<false, false, false, false, true>" },
      { ftgp_step_kernel<false, false, true, false, true>, "ftgp_step_kernel<false, false, true, false, true>" } },
    { { ftgp_step_kernel<true, false, false, false, true>, "ftgp_step_kernel<true, false, false, false, true>" },
      { ftgp_step_kernel<true, false, true, false, true>, "ftgp_step_kernel<true, false, true, false, true>" } } },
  { { { ftgp_step_kernel<false, false, false, true, true>, "ftgp_step_kernel<false, false, false, true, true>" },
      { ftgp_step_kernel<false, false, true, true, true>, "ftgp_step_kernel<false, false, true, true, true>" } },
    { { ftgp_step_kernel<true, false, false, true, true>, "ftgp_step_kernel<true, false, false, true, true>" },
      { ftgp_step_kernel<true, false, true, true, true>, "ftgp_step_kernel<true, false, true, true, true>" } } },
};

// ftgp_step_kernel<MULTI, false, true, TRACKS, DYN, true>: launches that name a network driver (ftgp_set_net)
const StepKernel kStepKernelsNet[2][2][2] = {   // [multi-track][multi][dynamics table]
  { { { ftgp_step_kernel<false, false, true, false, false, true>, "ftgp_step_kernel<false, false, true, false, false, true>" },
      { ftgp_step_kernel<false, false, true, false, true, true>, "ftgp_step_kernel<false, false, true, false, true, true>" } },
    { { ftgp_step_kernel<true, false, true, false, false, true>, "ftgp_step_kernel<true, false, true, false, false, true>" },
      { ftgp_step_kernel<true, false, true, false, true, true>, "ftgp_step_kernel<true, false, true, false, true, true>" } } },
  { { { ftgp_step_kernel<false, false, true, true, false, true>, "ftgp_step_kernel<false, false, true, true, false, true>" },
      { ftgp_step_kernel<false, false, true, true, true, true>, "ftgp_step_kernel<false, false, true, true, true, true>" } },
    { { ftgp_step_kernel<true, false, true, true, false, true>, "ftgp_step_kernel<true, false, true, true, false, true>" },
      { ftgp_step_kernel<true, false, true, true, true, true>, "ftgp_step_kernel<true, false, true, true, true, true>" } } },
};

const StepKernel& step_kernel(const FtgpEnv* e, bool roster, bool net = false)
{
    if (net) return kStepKernelsNet[e->n_tracks > 1][e->multi][e->dyn_on];           // (never a FAKELIDAR handle: ftgp_set_net refuses it)
    if (e->dyn_on) return kStepKernelsDyn[e->n_tracks > 1][e->multi][roster];      // (never a FAKELIDAR handle: the setters refuse it)
    return kStepKernels[e->n_tracks > 1][e->multi][e->P.lidar_mode == FTGP_LIDAR_FAKELIDAR ? 2 : roster ? 1 : 0];
}

// This rank's record of the launch (or metrics kernel) that wrote `slot`, once its event has been waited for: the record itself, or the
// sum of the workgroups' partial records (sums of integers, a minimum and a maximum: exact in any order -- bit-identical to what the
// step kernel's last workgroup or ftgp_metrics_kernel compute on the device).
void collect_slot(const FtgpEnv* e, int slot, double* out)
{
    if (!e->slot_partial[slot]) { memcpy(out, e->h_metrics.get() + (size_t)slot * FTGP_METRIC_DOUBLES, sizeof(double) * FTGP_METRIC_DOUBLES); return; }
    double v[FTGP_METRIC_DOUBLES] = { 0, 0, 0, 0, 0, 0, INFINITY, -INFINITY };
    const double* r = e->h_wg_metrics.get() + (size_t)slot * e->grid * FTGP_METRIC_DOUBLES;
    for (int b = 0; b < e->grid; ++b, r += FTGP_METRIC_DOUBLES) {
        for (int q = 0; q < 6; ++q) v[q] += r[q];
        v[6] = fmin(v[6], r[6]); v[7] = fmax(v[7], r[7]);
    }
    memcpy(out, v, sizeof v);
}

// The params block holds the slot table of the next FTGP_POLICY_PER_CAR launch: 0 = the user's roster, 1 = the device-io table.  A
// stream-ordered copy from pinned memory when it is the other one.
int use_table(FtgpEnv* e, int which)
{
    if (e->table_on_device == which) return 0;
    for (const TrackBufs& t : e->trk)     // every track's parameter block
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<unsigned char*>(e->d_params.get()) + t.block + offsetof(DeviceParams, car_policy), e->h_tables.get() + which * FTGP_MAX_CARS_PER_BLOCK,
                               sizeof e->P.car_policy, hipMemcpyHostToDevice, e->stream.get()));
    e->table_on_device = which;
    return 0;
}

// The network drivers a launch or a ftgp_policy_eval with `policy` names: bit s = slot s.  FTGP_POLICY_PER_CAR: those of the slot table
// it would run with (device_io: the device-io table).
unsigned nets_named(const FtgpEnv* e, int policy, bool device_io)
{
    if (is_net_policy(policy)) return 1u << (policy - FTGP_POLICY_NET0);
    if (policy != FTGP_POLICY_PER_CAR) return 0;
    const int32_t* table = device_io ? e->h_tables.get() + FTGP_MAX_CARS_PER_BLOCK : e->P.car_policy;
    unsigned m = 0;
    for (int k = 0; k < e->P.cars_per_env; ++k) if (is_net_policy(table[k])) m |= 1u << (table[k] - FTGP_POLICY_NET0);
    return m;
}
int check_nets_defined(const FtgpEnv* e, unsigned named)
{
    for (int s = 0; s < FTGP_MAX_NETS; ++s)
        if ((named >> s & 1u) && !e->slots[s].net.defined) return failf(FTGP_ERR_STATE, "FTGP_POLICY_NET%d: network slot %d is not defined (ftgp_set_net)", s, s);
    return 0;
}

// The preamble of every entry that names a network slot: the handle, the slot's range, and what the entry needs of the slot, looked at in
// this order; S is the slot, or the call is refused in the entry's name.  An entry that checks other arguments between two of these calls
// it twice.  instead: the entry to call on a slot that carries a population.
enum : unsigned { kSlotDefined = 1, kSlotValue = 2, kSlotPopulation = 4, kSlotNoPopulation = 8, kSlotTrainer = 16, kSlotNoTrainer = 32 };
int net_slot(FtgpEnv* e, const char* entry, int slot, unsigned needs, FtgpEnv::NetSlot*& S, const char* instead = nullptr)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (slot < 0 || slot >= FTGP_MAX_NETS) return failf(FTGP_ERR_ARG, "%s: slot = %d outside 0 .. %d", entry, slot, FTGP_MAX_NETS - 1);
    S = &e->slots[slot];
    if ((needs & kSlotDefined) && !S->net.defined) return failf(FTGP_ERR_STATE, "%s: network slot %d is not defined (ftgp_set_net)", entry, slot);
    if ((needs & kSlotValue) && !S->vnet.defined) return failf(FTGP_ERR_STATE, "%s: network slot %d has no value net (ftgp_set_value_net)", entry, slot);
    if ((needs & kSlotPopulation) && !S->pop_members) return failf(FTGP_ERR_STATE, "%s: network slot %d carries no population (ftgp_set_net_population)", entry, slot);
    if ((needs & kSlotNoPopulation) && S->pop_members)
        return failf(FTGP_ERR_STATE, "%s: network slot %d carries a population of %d members%s%s%s", entry, slot, S->pop_members, instead ? " (" : "", instead ? instead : "", instead ? ")" : "");
    if ((needs & kSlotTrainer) && !S->trainer.on) return failf(FTGP_ERR_STATE, "%s: network slot %d has no trainer (ftgp_train_begin)", entry, slot);
    if ((needs & kSlotNoTrainer) && S->trainer.on) return failf(FTGP_ERR_STATE, "%s: network slot %d has a trainer already (ftgp_train_end)", entry, slot);
    return 0;
}

// device_io: the launch of ftgp_step_device (the device-io slot table; checked by ftgp_device_io_config)
int launch_steps(FtgpEnv* e, int policy, int n_steps, bool device_io = false)
{
    e->rows_valid = false;
    if (n_steps < 0) return fail(FTGP_ERR_ARG, "n_steps < 0%s");
    const unsigned named = nets_named(e, policy, device_io);
    if (int rc = check_nets_defined(e, named)) return rc;
    if (!device_io) {
        if (policy == FTGP_POLICY_PER_CAR && !e->P.car_policy[0]) return fail(FTGP_ERR_STATE, "FTGP_POLICY_PER_CAR without ftgp_set_car_policies%s");
        if (uses_disparity_driver(e, policy)) if (int rc = check_disparity_shape(e->P)) return rc;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (policy == FTGP_POLICY_PER_CAR && n_steps > 0 && e->h_tables) if (int rc = use_table(e, device_io ? 1 : 0)) return rc;
    const int blocks = e->grid;
    const int slot = e->cur_slot ^ 1;
    // an exchange that is still reading this launch's slot (begin without end, two launches ago) goes first: over RCCL on the device (the
    // side stream's event); with one rank the "exchange" is the record in pinned memory, which is put aside before the slot is reused
    if (n_steps > 0 && e->gather_open && e->gather_slot == slot) {
        if (e->comm) HIP_TRY(hipStreamWaitEvent(e->stream.get(), e->ev_gather.get(), 0));
        else if (!e->gather_held) {
            // Waiting for an event of a launch is a blocked wait.  Polling hipEventQuery instead was measured (tools/launch_host.sh, round 4):
            // 7 us SLOWER per launch -- every query takes the runtime's locks and walks the stream's command list.
            HIP_TRY(hipEventSynchronize(e->gather_event));
            collect_slot(e, slot, e->held);
            e->gather_held = true;
        }
    }
    // The launch's two events ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL): no marker packet before and after it,
    // and their difference is the kernel's time alone.  FTGP_LAUNCH_PLAIN=1: hipEventRecord on either side instead.
    const bool ext = e->ext_launch && n_steps > 0;
    if (!ext) HIP_TRY(hipEventRecord(e->ev_start.get(), e->stream.get()));
    if (n_steps > 0) {
        const dim3 grid(blocks), block(e->P.waves_per_block * FTGP_WAVE);
        // (with the table of per-car dynamics on, the cars' records lie behind the layout)
        const uint32_t lds = (uint32_t)e->P.lds_bytes + (e->dyn_on ? (uint32_t)(e->P.cars_per_block * FTGP_DYN_RECORD * sizeof(double)) : 0u);
        hipEvent_t ev0 = ext ? e->ev_start.get() : nullptr, ev1 = ext ? e->ev_stop[slot].get() : nullptr;
        const bool roster = policy == FTGP_POLICY_PER_CAR;
        e->last_roster = roster;
        e->last_net = named != 0;
        // one rank and no communicator: the workgroups' partial records go straight to pinned host memory (bit 1 of the slot argument)
        const bool partial = e->h_wg_metrics != nullptr && e->comm == nullptr && e->d_wg_metrics != nullptr;
        const int slot_arg = slot | (partial ? 2 : 0);
        e->slot_partial[slot] = partial;
        hipExtLaunchKernelGGL(step_kernel(e, roster, named != 0).fn, grid, block, lds, e->stream.get(), ev0, ev1, 0, e->d_params.get(), policy, n_steps, slot_arg);
        HIP_TRY(hipGetLastError());
        e->cur_slot = slot;
        e->launch_metrics_valid = e->d_wg_metrics != nullptr;
    }
    if (!ext) HIP_TRY(hipEventRecord(e->ev_stop[e->cur_slot].get(), e->stream.get()));
    e->timed = true;
    return 0;
}

// packed read-back rows (one small kernel + two small copies instead of the whole state records)
int sync_rows_to_host(FtgpEnv* e)
{
    if (e->rows_valid) return 0;      // a host-driver step reads snapshot, progress and lap times: one pack, not three
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->P.n_cars;
    e->h_prog.resize(n * FTGP_PROGRESS_INTS); e->h_core.resize(n * kCoreDoubles);
    hipLaunchKernelGGL(ftgp_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream.get(), e->P, e->d_prog.get(), e->d_core.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e->h_prog.data(), e->d_prog.get(), sizeof(int32_t) * e->h_prog.size(), hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipMemcpyAsync(e->h_core.data(), e->d_core.get(), sizeof(double) * e->h_core.size(), hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    e->rows_valid = true;
    return 0;
}

// A caller's buffer of entry `entry`: `bytes` of device memory on the handle's device from p on (hipPointerGetAttributes, and the extent of
// the allocation from hipMemGetAddressRange); a refusal names the entry and the buffer.  Buffers found valid are remembered, so that the
// steady state asks the runtime nothing.
int check_device_buffer(FtgpEnv* e, const char* entry, const void* p, size_t bytes, const char* name)
{
    if (!p) return failf(FTGP_ERR_ARG, "%s: %s is NULL", entry, name);
    auto& ds = e->ds;
    for (const auto& c : ds.checked) if (c.p == p && c.bytes >= bytes) return 0;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return failf(FTGP_ERR_ARG, "%s: %s is not device memory", entry, name);
    }
    if (a.type != hipMemoryTypeDevice || a.device != e->device) return failf(FTGP_ERR_ARG, "%s: %s is not device memory on the handle's device", entry, name);
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return failf(FTGP_ERR_ARG, "%s: the allocation of %s is unknown to the runtime", entry, name);
    }
    const uintptr_t b = (uintptr_t)base, q = (uintptr_t)p;
    if (q < b || q - b + bytes > size) return failf(FTGP_ERR_ARG, "%s: %s is smaller than the layout needs", entry, name);
    ds.checked[ds.checked_next] = { p, bytes };
    ds.checked_next = (ds.checked_next + 1) % (int)(sizeof ds.checked / sizeof ds.checked[0]);
    return 0;
}

// ... of `count` elements of `each` bytes, in size_t: a product that does not fit is a buffer too small
int check_device_buffer(FtgpEnv* e, const char* entry, const void* p, size_t count, size_t each, const char* name)
{
    size_t bytes = 0;
    if (__builtin_mul_overflow(count, each, &bytes)) return failf(FTGP_ERR_ARG, "%s: %s is smaller than the layout needs", entry, name);
    return check_device_buffer(e, entry, p, bytes, name);
}

// the signals of the device step as the finish kernel takes them (ftgp_device_io_signals has checked s)
void set_signals(FtgpEnv* e, const FtgpDeviceSignals& s)
{
    DeviceSignalArgs& S = e->ds.sig;
    S = DeviceSignalArgs{};
    S.pool = s.scan_pool; S.n_beams = e->P.n_rays / s.scan_pool;
    S.vec_in = e->P.n_rays % 4 == 0;
    S.path = s.scan_pool >= FTGP_SIG_WAVE_POOL ? FTGP_SIG_PATH_WAVE
           : (S.vec_in && (s.scan_pool == 1 || s.scan_pool == 2 || s.scan_pool == 4)) ? FTGP_SIG_PATH_REGS : FTGP_SIG_PATH_STAGE;
    S.chunk_beams = (FTGP_SIG_STAGE_FLOATS / s.scan_pool) & ~3;
    S.clip = s.scan_max_range > 0.0f;
    S.limit = S.clip ? s.scan_max_range : INFINITY;
    S.inv_max_range = S.clip ? 1.0f / s.scan_max_range : 0.0f;
    S.terminate_off_track = s.terminate_off_track ? 1 : 0;
    S.penalty = s.off_track_penalty;
    e->ds.sig_default = s.scan_pool == 1 && !S.clip && !S.terminate_off_track && s.off_track_penalty == 0.0f;
}

// ftgp_io_contact_kernel on the handle's stream: every car's row to `rows` and / or the external cars' rows to `ext_out`
int launch_contacts(FtgpEnv* e, float* rows, float* ext_out)
{
    DeviceContactArgs C{};
    C.blocks = reinterpret_cast<const unsigned char*>(e->d_params.get());
    C.env_track = e->d_env_track.get();
    C.rows = rows; C.ext_out = ext_out;
    C.n_ext = e->ds.io.n_ext;
    for (int k = 0; k < FTGP_PAIR_STRIDE; ++k) C.ext_index[k] = e->ds.ready ? e->ds.io.ext_index[k] : -1;
    for (size_t k = 0; k < e->trk.size() && k < FTGP_MAX_TRACKS; ++k) C.block_off[k] = (uint32_t)e->trk[k].block;
    const unsigned blocks = (unsigned)(((size_t)e->P.n_cars * FTGP_CONTACT_LANES + FTGP_CONTACT_THREADS - 1) / FTGP_CONTACT_THREADS);
    hipLaunchKernelGGL(ftgp_io_contact_kernel, dim3(blocks), dim3(FTGP_CONTACT_THREADS), 0, e->stream.get(), e->P, C);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ensure_contact_rows(FtgpEnv* e)
{
    if (!e->ds.d_contact) HIP_TRY(dev_alloc(e->ds.d_contact, sizeof(float) * FTGP_CONTACT_FLOATS * (size_t)e->P.n_cars));
    return 0;
}

// ftgp_io_frame_kernel on the handle's stream: every car's row to `rows` and / or the external cars' rows to `ext_out`, s and the
// flags to slot `slot` of d_frame_s / d_frame_flag (-1: nowhere), with `want_c` the nearest points to that slot of d_frame_c
int launch_frame(FtgpEnv* e, int n_ahead, int stride, float* rows, float* ext_out, int slot, bool want_c = false)
{
    DeviceFrameArgs F{};
    F.env_track = e->d_env_track.get();
    F.rows = rows; F.ext_out = ext_out;
    F.s_out = slot >= 0 ? e->ds.d_frame_s.get() + (size_t)slot * (size_t)e->P.n_cars : nullptr;
    F.flag_out = slot >= 0 ? e->ds.d_frame_flag.get() + (size_t)slot * (size_t)e->P.n_cars : nullptr;
    F.c_out = slot >= 0 && want_c ? e->ds.d_frame_c.get() + (size_t)slot * (size_t)e->P.n_cars : nullptr;
    F.n_ext = e->ds.io.n_ext; F.n_ahead = n_ahead; F.stride = stride;
    for (int k = 0; k < FTGP_PAIR_STRIDE; ++k) F.ext_index[k] = e->ds.ready ? e->ds.io.ext_index[k] : -1;
    const unsigned blocks = (unsigned)(((size_t)e->P.n_cars * FTGP_FRAME_LANES + FTGP_FRAME_THREADS - 1) / FTGP_FRAME_THREADS);
    hipLaunchKernelGGL(ftgp_io_frame_kernel, dim3(blocks), dim3(FTGP_FRAME_THREADS), 0, e->stream.get(), e->P, F);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the two slots of (s, flags) that a launch_frame with a slot writes
int ensure_frame_slots(FtgpEnv* e)
{
    const size_t n_cars = (size_t)e->P.n_cars;
    if (!e->ds.d_frame_s) HIP_TRY(dev_alloc(e->ds.d_frame_s, sizeof(double) * 2 * n_cars));
    if (!e->ds.d_frame_flag) HIP_TRY(dev_alloc(e->ds.d_frame_flag, sizeof(int32_t) * 2 * n_cars));
    return 0;
}

int ensure_frame_rows(FtgpEnv* e)
{
    const size_t n_cars = (size_t)e->P.n_cars;
    if (!e->ds.d_frame) HIP_TRY(dev_alloc(e->ds.d_frame, sizeof(float) * (FTGP_FRAME_FIXED + 2 * FTGP_MAX_LOOKAHEAD) * n_cars));
    return ensure_frame_slots(e);
}

// ftgp_io_rival_kernel on the handle's stream, behind a launch_frame(.., slot, true) at the same records: every car's row to `rows`
// and / or the external cars' rows to `ext_out`, or (places_only) nothing but the places to d_place0
int launch_rivals(FtgpEnv* e, int n_rivals, float* rows, float* ext_out, int slot, bool places_only = false)
{
    const size_t at = (size_t)slot * (size_t)e->P.n_cars;
    DeviceRivalArgs V{};
    V.s = e->ds.d_frame_s.get() + at; V.c = e->ds.d_frame_c.get() + at; V.flag = e->ds.d_frame_flag.get() + at;
    V.rows = rows; V.ext_out = ext_out;
    V.place_out = places_only ? e->ds.d_place0.get() : nullptr;
    V.n_ext = e->ds.io.n_ext; V.n_rivals = n_rivals;
    for (int k = 0; k < FTGP_PAIR_STRIDE; ++k) V.ext_index[k] = e->ds.ready ? e->ds.io.ext_index[k] : -1;
    const unsigned blocks = (unsigned)(((size_t)e->P.n_cars * FTGP_RIVAL_LANES + FTGP_RIVAL_THREADS - 1) / FTGP_RIVAL_THREADS);
    hipLaunchKernelGGL(ftgp_io_rival_kernel, dim3(blocks), dim3(FTGP_RIVAL_THREADS), 0, e->stream.get(), e->P, V);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ensure_rival_rows(FtgpEnv* e)
{
    const size_t n_cars = (size_t)e->P.n_cars;
    if (!e->ds.d_rival) HIP_TRY(dev_alloc(e->ds.d_rival, sizeof(float) * (FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * FTGP_MAX_RIVALS) * n_cars));
    if (!e->ds.d_frame_c) HIP_TRY(dev_alloc(e->ds.d_frame_c, sizeof(int32_t) * 2 * n_cars));
    if (!e->ds.d_place0) HIP_TRY(dev_alloc(e->ds.d_place0, sizeof(int32_t) * n_cars));
    return ensure_frame_slots(e);
}

// the search and the rival kernel at the current records: the two launches of ftgp_rivals_device and ftgp_get_rivals
int launch_rivals_now(FtgpEnv* e, int n_rivals, float* rows, float* ext_out)
{
    if (int rc = launch_frame(e, 0, 1, nullptr, nullptr, 1, true)) return rc;
    return launch_rivals(e, n_rivals, rows, ext_out, 1);
}

// stream `behind` waits for what stream `ahead` holds so far, through event ev
int stream_waits_for(hipStream_t behind, hipStream_t ahead, const Event& ev)
{
    HIP_TRY(hipEventRecord(ev.get(), ahead));
    HIP_TRY(hipStreamWaitEvent(behind, ev.get(), 0));
    return 0;
}

// The fence of every entry that works on the handle's stream for a caller's: the handle's stream waits for what the caller's holds, `work`
// enqueues on the handle's stream, and the caller's stream waits for that.  Safe as a handle's first call: the two events are made here.
// An entry validates before it comes here, so nothing is enqueued for a refused call; if `work` fails, its code is returned without the
// closing fence.
template <class Work>
int on_handle_stream(FtgpEnv* e, void* caller_stream, Work work)
{
    hipStream_t caller = (hipStream_t)caller_stream;
    if (!e->ds.ev_in) HIP_TRY(make_event(e->ds.ev_in, hipEventDisableTiming));
    if (!e->ds.ev_out) HIP_TRY(make_event(e->ds.ev_out, hipEventDisableTiming));
    if (int rc = stream_waits_for(e->stream.get(), caller, e->ds.ev_in)) return rc;
    if (int rc = work()) return rc;
    return stream_waits_for(caller, e->stream.get(), e->ds.ev_out);
}

// ftgp_state_device, ftgp_contacts_device, ftgp_frame_device, ftgp_rivals_device, ftgp_obs_device (`entry`): the external agents' rows of `floats` floats,
// written by `launch` on the handle's stream to the caller's buffer `out` (`name` in a refusal)
template <class Launch>
int rows_to_device(FtgpEnv* e, const char* entry, void* stream, size_t floats, float* out, const char* name, Launch launch)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!e->ds.ready) return fail(FTGP_ERR_STATE, "%s before ftgp_device_io_config", entry);
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = check_device_buffer(e, entry, out, sizeof(float) * floats * (size_t)e->P.n_envs * (size_t)e->ds.io.n_ext, name)) return rc;
    return on_handle_stream(e, stream, launch);
}

// The first setter call of a handle: the DYN kernels may use the LDS the others may, the records are allocated (zeroed, the counter with
// them) and every parameter block learns their address.  ftgp_create does nothing for the table: a handle that never sets one is, on the
// host and on the device, the handle it always was.
int ensure_dynamics(FtgpEnv* e)
{
    if (e->d_dyn) return 0;
    for (const auto& set : kStepKernelsDyn) for (const auto& row : set) for (const StepKernel& k : row) HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the blocks while they change
    DevBuf<double> d;
    HIP_TRY(dev_alloc(d, FTGP_DYN_BYTES(e->P.n_cars)));
    HIP_TRY(hipMemset(d.get(), 0, FTGP_DYN_BYTES(e->P.n_cars)));
    const uint64_t a = (uint64_t)(uintptr_t)d.get();
    const uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
    for (const TrackBufs& t : e->trk) {   // every track's parameter block
        unsigned char* block = reinterpret_cast<unsigned char*>(e->d_params.get()) + t.block;
        HIP_TRY(hipMemcpy(block + offsetof(DeviceParams, dyn_table_lo), &lo, sizeof lo, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(block + offsetof(DeviceParams, dyn_table_hi), &hi, sizeof hi, hipMemcpyHostToDevice));
    }
    e->P.dyn_table_lo = lo; e->P.dyn_table_hi = hi;
    e->d_dyn = std::move(d);
    return 0;
}

// ftgp_set_dynamics / ftgp_set_dynamics_device: ftgp_dynamics_kernel on the handle's stream; the first launch since the table was off
// also gives every car the handle's own row
// (env_mask_or: with env_mask, an env is taken if either byte is set -- the terminated | truncated of a collected decision)
int launch_dynamics(FtgpEnv* e, const double* rows, const uint8_t* env_mask, const uint8_t* env_mask_or = nullptr)
{
    if (int rc = ensure_dynamics(e)) return rc;
    DynArgs A = e->dyn;
    A.init = e->dyn_on ? 0 : 1; A.rows = rows; A.env_mask = env_mask; A.env_mask_or = env_mask_or;
    hipLaunchKernelGGL(ftgp_dynamics_kernel, dim3((unsigned)((e->P.n_cars + 255) / 256)), dim3(256), 0, e->stream.get(), e->P, A);
    HIP_TRY(hipGetLastError());
    e->dyn_on = true;
    return 0;
}

// the track fingerprint of an env-state record (include/ftgp.h): a splitmix64 fold over the size, the wall bitmap and the centre-line
uint64_t track_fingerprint(int width, int height, const std::vector<uint32_t>& bits, const std::vector<double>& path)
{
    uint64_t h = 0;
    auto fold = [&h](uint64_t v) { h = splitmix64(h ^ v); };
    fold((uint64_t)width); fold((uint64_t)height);
    for (const uint32_t w : bits) fold((uint64_t)w);
    for (int i = 0; i < 2 * FTGP_PATH_POINTS; ++i) { uint64_t b; memcpy(&b, &path[(size_t)i], sizeof b); fold(b); }
    return h;
}

// bytes of one env-state record, and its scan rows in uint4
size_t env_state_row_vec(const DeviceParams& P) { return ((size_t)P.n_rays * sizeof(float) + 15) / 16; }
size_t env_state_bytes(const DeviceParams& P)
{
    return 16 * (FTGP_ENV_STATE_HEAD + (size_t)P.cars_per_env * ((size_t)FTGP_CAR_VEC + FTGP_DYN_VEC + env_state_row_vec(P)));
}

// A handle's first save or load: the handle's own dynamics record, a zeroed counter and the fingerprints go to device memory.
int ensure_env_state(FtgpEnv* e)
{
    if (e->d_state_aux) return 0;
    EnvStateAux a{};
    memcpy(a.own, e->dyn.base, sizeof e->dyn.base);
    for (int r = 0; r < 4; ++r) a.own[kDynWheelLoad + r] = e->P.wheel_load[r];
    for (size_t k = 0; k < e->track_fp.size() && k < FTGP_MAX_TRACKS; ++k) a.track_fp[k] = e->track_fp[k];
    HIP_TRY(dev_upload(e->d_state_aux, &a, sizeof a));
    return 0;
}

// the arguments both env-state kernels take, and their launch shape: a wave per env
EnvStateArgs env_state_args(FtgpEnv* e, void* rows, int64_t n_rows)
{
    EnvStateArgs A{};
    A.rows = static_cast<uint4*>(rows); A.n_rows = n_rows;
    A.env_track = e->d_env_track.get(); A.aux = e->d_state_aux.get(); A.episodes = e->d_episodes.get();
    A.dyn = e->dyn_on ? reinterpret_cast<uint4*>(dyn_table(&e->P)) : nullptr;
    A.row_vec = (int32_t)env_state_row_vec(e->P); A.env_vec = (int32_t)(env_state_bytes(e->P) / 16);
    return A;
}
unsigned env_state_blocks(const FtgpEnv* e) { const int per = FTGP_ENV_STATE_THREADS / FTGP_WAVE; return (unsigned)((e->P.n_envs + per - 1) / per); }

bool nonneg_finite(double v) { return v >= 0.0 && !std::isinf(v); }      // a penalty, a range, a margin; a NaN fails as well

// ftgp_create, step 3: the upload -- allocate, copy, search the box fields (or the distance transforms), write the images
int upload(FtgpEnv* e, const Plan& pl, const Switches& sw)
{
    const DeviceParams& P = pl.tracks[0].P;         // the batch's values (e->P: track 0's finished block, at the end)
    hipStream_t s = e->stream.get();
    const int T = (int)pl.tracks.size();
    const size_t n_cars = (size_t)P.n_cars;
    e->n_tracks = T;
    e->trk.resize((size_t)T);
    if (P.lidar_mode == FTGP_LIDAR_FAKELIDAR) HIP_TRY(dev_upload(e->d_fan, pl.fan.data(), pl.fan.size() * sizeof(double)));
    for (int k = 0; k < T; ++k) {
        const DeviceParams& Q = pl.tracks[(size_t)k].P;
        const HostTables& tab = pl.tracks[(size_t)k].tab;
        TrackBufs& b = e->trk[(size_t)k];
        b.width = Q.width; b.height = Q.height;
        const size_t plane = (size_t)Q.width * Q.height;
        size_t field_bytes = 0;
        if (P.lidar_mode == FTGP_LIDAR_FAKELIDAR) {
            // The distance transform of custom.py:1149-1153 / raycast.py:24-27 (scipy.ndimage.distance_transform_edt of the non-wall
            // mask) without scipy, exact: the squared distance is the minimum over the columns x' of (x - x')^2 + g(x', y)^2 with g the
            // vertical distance to the nearest wall of column x' -- the run lengths above -- in integers; one correctly rounded sqrt.
            DevBuf<uint16_t> d_runy;
            HIP_TRY(dev_upload(d_runy, tab.runy.data(), 2 * plane * sizeof(uint16_t)));
            field_bytes = plane * sizeof(double);
            HIP_TRY(dev_alloc(b.edt, field_bytes));
            hipLaunchKernelGGL(ftgp_edt_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, d_runy.get(), Q.width, Q.height, b.edt.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
        } else {   // sector box field: upload the run lengths, search the boxes on the device
            const size_t plane_cells = (size_t)Q.plane256 * 128;
            DevBuf<uint16_t> d_runx, d_runy;
            field_bytes = plane_cells * (size_t)Q.n_planes * sizeof(uint16_t);
            HIP_TRY(dev_alloc(b.field, field_bytes));
            HIP_TRY(dev_upload(d_runx, tab.runx.data(), 2 * plane * sizeof(uint16_t)));
            HIP_TRY(dev_upload(d_runy, tab.runy.data(), 2 * plane * sizeof(uint16_t)));
            hipLaunchKernelGGL(ftgp_box_field_kernel, dim3((unsigned)((plane_cells * Q.n_sectors + 255) / 256)), dim3(256), 0, s, d_runx.get(), d_runy.get(), Q.width, Q.height, Q.n_sectors, b.field.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
        }
        const size_t sz_bits = sizeof(uint32_t) * (size_t)Q.height * Q.words_per_row;
        HIP_TRY(dev_upload(b.bits, tab.bits.data(), sz_bits));
        HIP_TRY(dev_upload(b.nearbits, tab.nearbits.data(), sz_bits));
        if (sw.verbose)
            fprintf(stderr, "ftgp_create: track %d: %d x %d px, %.1f MB of %s + %.1f MB of wall bitmaps\n", k, Q.width, Q.height, field_bytes / 1e6,
                    P.lidar_mode == FTGP_LIDAR_FAKELIDAR ? "distance transform" : "box field", 2.0 * sz_bits / 1e6);
    }
    const size_t sz_path = sizeof(double) * 2 * FTGP_PATH_POINTS, sz_spawn = sizeof(double) * 4 * FTGP_PATH_POINTS;
    {   // centre-lines and spawn tables of all tracks, track after track
        std::vector<double> paths(2 * FTGP_PATH_POINTS * (size_t)T), spawns(4 * FTGP_PATH_POINTS * (size_t)T);
        for (int k = 0; k < T; ++k) {
            memcpy(paths.data() + 2 * FTGP_PATH_POINTS * (size_t)k, pl.tracks[(size_t)k].path.data(), sz_path);
            memcpy(spawns.data() + 4 * FTGP_PATH_POINTS * (size_t)k, pl.tracks[(size_t)k].spawn.data(), sz_spawn);
        }
        HIP_TRY(dev_upload(e->d_path, paths.data(), sz_path * T));
        HIP_TRY(dev_upload(e->d_spawn, spawns.data(), sz_spawn * T));
        e->start_table.assign(6 * FTGP_PATH_POINTS * (size_t)T, 0.0);
        for (int k = 0; k < T; ++k)
            for (int p = 0; p < FTGP_PATH_POINTS; ++p) {
                double* row = &e->start_table[6 * (FTGP_PATH_POINTS * (size_t)k + p)];
                memcpy(row, &pl.tracks[(size_t)k].spawn[4 * (size_t)p], sizeof(double) * 4);
                memcpy(row + 4, &pl.tracks[(size_t)k].clear[2 * (size_t)p], sizeof(double) * 2);
            }
    }
    e->track_fp.clear();
    for (int k = 0; k < T; ++k) e->track_fp.push_back(track_fingerprint(pl.tracks[(size_t)k].P.width, pl.tracks[(size_t)k].P.height, pl.tracks[(size_t)k].tab.bits, pl.tracks[(size_t)k].path));
    HIP_TRY(dev_upload(e->d_veh, pl.veh.data(), pl.veh.size()));
    HIP_TRY(dev_upload(e->d_ray, pl.ray.data(), sizeof(float) * pl.ray.size()));
    HIP_TRY(dev_upload(e->d_cover, pl.cover.data(), sizeof(float) * pl.cover.size()));
    if (T > 1) HIP_TRY(dev_upload(e->d_env_track, pl.env_track.data(), sizeof(int32_t) * pl.env_track.size()));
    // zeroed on the handle's own stream: a non-blocking stream is not ordered against the null stream, and ftgp_reset() runs on it
    HIP_TRY(dev_zeros(e->d_cars, sizeof(CarState) * n_cars, s)); HIP_TRY(dev_zeros(e->d_ranges, sizeof(float) * n_cars * P.ranges_stride, s));
    HIP_TRY(dev_zeros(e->d_steps, sizeof(int64_t) * (size_t)P.n_envs, s)); HIP_TRY(dev_alloc(e->d_env_mask, (size_t)P.n_envs)); HIP_TRY(dev_alloc(e->d_car_mask, n_cars));
    HIP_TRY(dev_alloc(e->d_ctrl, sizeof(double) * 2 * n_cars)); HIP_TRY(dev_alloc(e->d_pose, sizeof(double) * FTGP_POSE_DOUBLES * n_cars));
    HIP_TRY(dev_alloc(e->d_metrics, sizeof(double) * FTGP_METRIC_DOUBLES * 2));
    HIP_TRY(host_alloc(e->h_metrics, sizeof(double) * FTGP_METRIC_DOUBLES * 2, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void**)&e->h_metrics_dev, e->h_metrics.get(), 0));
    e->grid = pl.n_wg;
    double* wg_metrics_host = nullptr;
    if (!sw.no_fused_metrics) {          // (diagnostic switch: tests compare the fused record with ftgp_metrics_kernel's)
        const size_t blocks = (size_t)pl.n_wg;
        HIP_TRY(dev_alloc(e->d_wg_metrics, sizeof(double) * FTGP_METRIC_DOUBLES * blocks));
        HIP_TRY(dev_zeros(e->d_wg_ticket, sizeof(unsigned int), s));
        if (!sw.no_host_sum) {           // (diagnostic switch: the device-side hand-off of the record also with one rank)
            HIP_TRY(host_alloc(e->h_wg_metrics, sizeof(double) * FTGP_METRIC_DOUBLES * 2 * blocks, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void**)&wg_metrics_host, e->h_wg_metrics.get(), 0));
        }
    }
    HIP_TRY(dev_alloc(e->d_prog, sizeof(int32_t) * FTGP_PROGRESS_INTS * n_cars)); HIP_TRY(dev_alloc(e->d_core, sizeof(double) * kCoreDoubles * n_cars));
    // the two images, laid out for the addresses just allocated
    const ImageSizes z = image_sizes(pl);
    HIP_TRY(dev_alloc(e->d_params, z.params));
    HIP_TRY(dev_alloc(e->d_stage, z.stage * T));
    DeviceAddrs a;
    for (const TrackBufs& b : e->trk) a.trk.push_back({ b.field.get(), b.edt.get(), b.bits.get(), b.nearbits.get() });
    a.fan = e->d_fan.get(); a.path = e->d_path.get(); a.spawn = e->d_spawn.get(); a.veh = e->d_veh.get(); a.ray = e->d_ray.get(); a.cover = e->d_cover.get();
    a.cars = e->d_cars.get(); a.ranges = e->d_ranges.get(); a.steps = e->d_steps.get();
    if (e->d_wg_metrics) { a.wg_metrics = e->d_wg_metrics.get(); a.wg_ticket = e->d_wg_ticket.get(); a.metrics_dev = e->d_metrics.get(); a.metrics_host = e->h_metrics_dev; }
    a.wg_metrics_host = wg_metrics_host;
    a.params = reinterpret_cast<const unsigned char*>(e->d_params.get()); a.stage = e->d_stage.get();
    Images im;
    layout_images(pl, a, im);
    for (int k = 0; k < T; ++k) e->trk[(size_t)k].block = im.blocks[(size_t)k];
    memcpy(&e->P, &im.P0, sizeof e->P);         // as it lies, padding included
    {   // per-car dynamics: the handle's own row, and plan()'s wheel-load rule as factors of wtot (the same operands, divided once here)
        const FtgpVehicle& v = e->P.veh;
        const double base[FTGP_DYN_DOUBLES] = { v.mass, v.izz, v.friction, v.tire_damping, v.throttle_kv, v.throttle_force_limit, v.steer_kp, v.steer_damping };
        DynArgs& d = e->dyn;
        memcpy(d.base, base, sizeof base);
        d.gravity = v.gravity;
        if (v.kind == FTGP_VEHICLE_TRICYCLE) {
            const double a_f = v.wheel_x[2], a_r = -0.5 * (v.wheel_x[0] + v.wheel_x[1]);
            d.load_k[0] = d.load_k[1] = a_f / (a_f + a_r); d.load_half[0] = d.load_half[1] = 1;
            d.load_k[2] = a_r / (a_f + a_r); d.load_k[3] = 0.0; d.load_half[2] = d.load_half[3] = 0;
        } else {
            const double a_f = 0.5 * (v.wheel_x[0] + v.wheel_x[1]), a_r = -0.5 * (v.wheel_x[2] + v.wheel_x[3]);
            d.load_k[0] = d.load_k[1] = a_r / (a_f + a_r); d.load_k[2] = d.load_k[3] = a_f / (a_f + a_r);
            for (int r = 0; r < 4; ++r) d.load_half[r] = 1;
        }
    }
    HIP_TRY(hipMemcpy(e->d_stage.get(), im.stage.data(), im.stage.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_params.get(), im.params.data(), im.params.size(), hipMemcpyHostToDevice));
    return 0;
}

// ftgp_create / ftgp_create_tracks after the checks: device probe, plan, upload, reset
int create(const FtgpConfig& cfg, const FtgpTrack* tracks, const int32_t* envs_per_track, int n_tracks, const Switches& sw, FtgpEnv** out)
{
    if (int rc = open_device(cfg.device_id)) return rc;
    hipDeviceProp_t prop; HIP_TRY(hipGetDeviceProperties(&prop, cfg.device_id));
    const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    Plan pl;
    if (int rc = plan(cfg, tracks, envs_per_track, n_tracks, n_cu, sw, pl)) return rc;
    std::unique_ptr<FtgpEnv, int (*)(FtgpEnv*)> e(new FtgpEnv(), ftgp_destroy);
    e->device = cfg.device_id; e->multi = cfg.cars_per_env > 1; e->ext_launch = !sw.launch_plain;
    HIP_TRY(make_stream(e->stream)); HIP_TRY(make_stream(e->side));
    HIP_TRY(make_event(e->ev_start, hipEventDefault)); HIP_TRY(make_event(e->ev_stop[0], hipEventDefault)); HIP_TRY(make_event(e->ev_stop[1], hipEventDefault));
    HIP_TRY(make_event(e->ev_metrics, hipEventDisableTiming)); HIP_TRY(make_event(e->ev_gather, hipEventDisableTiming));
    for (const auto& set : kStepKernels) for (const auto& row : set) for (const StepKernel& k : row) HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (int rc = upload(e.get(), pl, sw)) return rc;
    if (int rc = ftgp_reset(e.get(), nullptr)) return rc;
    *out = e.release();
    return 0;
}

// One device step in two halves, shared by ftgp_step_device_rivals and ftgp_collect_device.  plan_device_step: every check of the call
// and the kernels' argument blocks; nothing is enqueued.  enqueue_device_step: the launches of one call on the handle's stream, without
// the fences to and from a caller's stream, with `between` run behind the steps' own kernels (launch_steps and the contact, frame and
// rival rows) and in front of the finish kernel, where an env that ended is reset.
struct DeviceStepPlan {
    DeviceIoArgs A; DeviceSignalArgs S;
    bool signals = false, dense = false, place = false, aligned = false;
};

int plan_device_step(FtgpEnv* e, const FtgpDeviceStep* io, const FtgpDeviceStepExtra* extra, const FtgpDeviceStepContacts* contacts,
                     const FtgpDeviceStepFrame* frame, const FtgpDeviceStepRivals* rivals, DeviceStepPlan& plan)
{
    if (!e || !io) return fail(FTGP_ERR_ARG, "null argument%s");
    FtgpEnv::DeviceStep& ds = e->ds;
    if (!ds.ready) return fail(FTGP_ERR_STATE, "ftgp_step_device before ftgp_device_io_config%s");
    if (int rc = check_nets_defined(e, nets_named(e, FTGP_POLICY_PER_CAR, true))) return rc;      // (before anything is enqueued)
    // the four optional kinds of rows: floats per row, the caller's two buffers and what a refusal calls them
    struct Rows { const char* name; const char* final_name; size_t floats; float* out; float* final_out; };
    const Rows st{ "state", "final_state", FTGP_STATE_FLOATS, extra ? extra->state : nullptr, extra ? extra->final_state : nullptr };
    const Rows ct{ "contact", "final_contact", FTGP_CONTACT_FLOATS, contacts ? contacts->contact : nullptr, contacts ? contacts->final_contact : nullptr };
    const Rows fr{ "frame", "final_frame", (size_t)(FTGP_FRAME_FIXED + 2 * ds.frame.n_ahead), frame ? frame->frame : nullptr, frame ? frame->final_frame : nullptr };
    const Rows rv{ "rival", "final_rival", (size_t)(FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * ds.rivals.n_rivals), rivals ? rivals->rival : nullptr, rivals ? rivals->final_rival : nullptr };
    if ((ct.out || ct.final_out) && !ds.con_on) return fail(FTGP_ERR_STATE, "ftgp_step_device_contacts: contact buffers while contacts are off (ftgp_device_io_contacts)%s");
    if ((fr.out || fr.final_out) && !ds.frame_on) return fail(FTGP_ERR_STATE, "ftgp_step_device_frame: frame buffers while the frame is off (ftgp_device_io_frame)%s");
    if ((rv.out || rv.final_out) && !ds.rivals_on) return fail(FTGP_ERR_STATE, "ftgp_step_device_rivals: rival buffers while rivals are off (ftgp_device_io_rivals)%s");
    HIP_TRY(hipSetDevice(e->device));
    DeviceIoArgs& A = plan.A;
    DeviceSignalArgs& S = plan.S;
    A = ds.io;
    S = ds.sig;
    S.state = st.out; S.final_state = st.final_out;
    plan.signals = !ds.sig_default || S.state || S.final_state || ds.con_on || ds.frame_on || ds.rivals_on;
    const size_t n_envs = (size_t)e->P.n_envs, rows = n_envs * (size_t)A.n_ext, obs_bytes = sizeof(float) * rows * (size_t)S.n_beams;
    if (int rc = check_device_buffer(e, "ftgp_step_device", io->action, sizeof(float) * 2 * rows, "action")) return rc;
    if (int rc = check_device_buffer(e, "ftgp_step_device", io->obs, obs_bytes, "obs")) return rc;
    if (int rc = check_device_buffer(e, "ftgp_step_device", io->reward, sizeof(float) * rows, "reward")) return rc;
    if (int rc = check_device_buffer(e, "ftgp_step_device", io->terminated, n_envs, "terminated")) return rc;
    if (int rc = check_device_buffer(e, "ftgp_step_device", io->truncated, n_envs, "truncated")) return rc;
    if (io->final_obs) if (int rc = check_device_buffer(e, "ftgp_step_device", io->final_obs, obs_bytes, "final_obs")) return rc;
    for (const Rows* r : { &st, &ct, &fr, &rv }) {
        if (r->out) if (int rc = check_device_buffer(e, "ftgp_step_device", r->out, sizeof(float) * r->floats * rows, r->name)) return rc;
        if (r->final_out) if (int rc = check_device_buffer(e, "ftgp_step_device", r->final_out, sizeof(float) * r->floats * rows, r->final_name)) return rc;
    }
    plan.dense = ds.frame_on && ds.frame.dense_progress != 0;
    if (ds.frame_on) {
        S.frame_rows = ds.d_frame.get(); S.frame = fr.out; S.final_frame = fr.final_out;
        S.frame_ahead = ds.frame.n_ahead; S.frame_stride = ds.frame.stride;
        if (plan.dense) {
            S.frame_s0 = ds.d_frame_s.get(); S.frame_s1 = ds.d_frame_s.get() + e->P.n_cars;
            S.frame_flag0 = ds.d_frame_flag.get(); S.frame_flag1 = ds.d_frame_flag.get() + e->P.n_cars;
        }
    }
    plan.place = ds.rivals_on && ds.rivals.place_weight != 0.0f;
    if (ds.rivals_on) {
        S.rival_rows = ds.d_rival.get(); S.rival = rv.out; S.final_rival = rv.final_out;
        S.rival_n = ds.rivals.n_rivals;
        if (plan.place) { S.place0 = ds.d_place0.get(); S.place_weight = ds.rivals.place_weight; }
    }
    if (ds.con_on) {
        S.contact_rows = ds.d_contact.get(); S.contact = ct.out; S.final_contact = ct.final_out;
        S.terminate_on_wall = ds.con.terminate_on_wall ? 1 : 0; S.terminate_on_car = ds.con.terminate_on_car ? 1 : 0;
        S.wall_penalty = ds.con.wall_penalty; S.car_penalty = ds.con.car_penalty;
    }
    A.action = io->action; A.obs = io->obs; A.reward = io->reward; A.terminated = io->terminated; A.truncated = io->truncated; A.final_obs = io->final_obs;
    A.vec4 = e->P.n_rays % 4 == 0 && (uintptr_t)io->obs % 16 == 0 && (uintptr_t)io->final_obs % 16 == 0;
    plan.aligned = (uintptr_t)io->obs % 16 == 0 && (uintptr_t)io->final_obs % 16 == 0;
    return 0;
}

template <class Between>
int enqueue_device_step(FtgpEnv* e, const DeviceStepPlan& plan, Between between)
{
    FtgpEnv::DeviceStep& ds = e->ds;
    const DeviceIoArgs& A = plan.A;
    const unsigned car_blocks = (unsigned)((e->P.n_cars + 255) / 256);
    hipLaunchKernelGGL(ftgp_io_ingest_kernel, dim3(car_blocks), dim3(256), 0, e->stream.get(), e->P, A);
    HIP_TRY(hipGetLastError());
    if (plan.dense || plan.place) if (int rc = launch_frame(e, 0, 1, nullptr, nullptr, 0, plan.place)) return rc;          // s0: the pose the call begins with
    if (plan.place) if (int rc = launch_rivals(e, 0, nullptr, nullptr, 0, true)) return rc;      // p0: the places the call begins with
    if (int rc = launch_steps(e, FTGP_POLICY_PER_CAR, ds.repeat, true)) return rc;
    if (ds.con_on) if (int rc = launch_contacts(e, ds.d_contact.get(), nullptr)) return rc;
    if (ds.frame_on) { if (int rc = launch_frame(e, ds.frame.n_ahead, ds.frame.stride, ds.d_frame.get(), nullptr, 1, ds.rivals_on)) return rc; }
    else if (ds.rivals_on) if (int rc = launch_frame(e, 0, 1, nullptr, nullptr, 1, true)) return rc;           // the rivals' own search
    if (ds.rivals_on) if (int rc = launch_rivals(e, ds.rivals.n_rivals, ds.d_rival.get(), nullptr, 1)) return rc;
    if (int rc = between()) return rc;
    if (!plan.signals) hipLaunchKernelGGL(ftgp_io_finish_kernel, dim3((unsigned)e->P.n_envs), dim3(FTGP_IO_THREADS), 0, e->stream.get(), e->P, A, e->rule);
    else {
        DeviceSignalArgs S = plan.S;
        S.vec_out = plan.aligned && S.n_beams % 4 == 0;
        if (S.path == FTGP_SIG_PATH_REGS && !plan.aligned) S.path = FTGP_SIG_PATH_STAGE;
        hipLaunchKernelGGL(ftgp_io_finish_signals_kernel, dim3((unsigned)e->P.n_envs), dim3(FTGP_IO_THREADS), 0, e->stream.get(), e->P, A, S, e->rule);
    }
    HIP_TRY(hipGetLastError());
    e->rows_valid = false;
    if (A.auto_reset) e->launch_metrics_valid = false;     // the launch's record describes the state before the resets
    return 0;
}

}  // namespace

extern "C" {

void ftgp_default_vehicle(FtgpVehicle* v)
{
    memset(v, 0, sizeof *v);
    // masses: chassis 3.542137 (mushr.em.xml:119) + 4 x 0.498952 (:69) + steering-wheel geom 0.01 (:122)
    // + LiDAR puck (cylinder r 0.03, half-height 0.015, default density 1000; :108) + softeners 4e-5 (:66)
    v->mass = 5.632768;
    v->izz = 0.0316994;              // yaw inertia of those parts about the body origin (chassis from the STL volume)
    const double s = 0.5;            // mushr_scale (:23)
    v->wheel_x[0] = s * 0.1385;  v->wheel_y[0] = s * 0.115;     // fl (:124)
    v->wheel_x[1] = s * 0.1385;  v->wheel_y[1] = s * -0.115;    // fr (:137)
    v->wheel_x[2] = s * -0.158;  v->wheel_y[2] = s * 0.115;     // bl (:150)
    v->wheel_x[3] = s * -0.158;  v->wheel_y[3] = s * -0.115;    // br (:162)
    v->wheel_radius = 0.03;
    v->wheel_inertia = 0.01 + 0.498952 / 5.0 * (0.03 * 0.03 + 0.03 * 0.03);   // armature + ellipsoid about its axle
    v->wheel_damping = 0.01;
    v->throttle_kv = 100.0; v->throttle_gear = 0.04; v->throttle_force_limit = 500.0;
    v->steer_kp = 20.0; v->steer_damping = 0.3;
    v->steer_inertia = 3 * 0.0002 + 2 * (0.498952 / 5.0 * (0.03 * 0.03 + 0.01 * 0.01)) + 0.01 / 5.0 * (0.03 * 0.03 + 0.01 * 0.01);
    v->steer_limit = 1.0;
    v->friction = 0.5; v->gravity = 9.81;
    v->tire_damping = (v->mass / 4.0) * (2.0 / (0.95 * 0.02));                 // solref 0.02, solimp dmax 0.95 (:69)
    v->contact_x[0] = 0.0385; v->contact_x[1] = 0.0; v->contact_x[2] = -0.0385;
    v->contact_radius = 0.0655;
    v->contact_stiffness = v->mass / (0.95 * 0.95 * 0.02 * 0.02);
    v->contact_damping = v->mass * (2.0 / (0.95 * 0.02));
    v->lidar_x = -0.0525; v->lidar_y = 0.0; v->lidar_ring_radius = 0.03;       // (:101-103)
    v->body_z = 0.0156;
    v->box_xmin = -0.1027; v->box_xmax = 0.1034; v->box_ymin = -0.0461; v->box_ymax = 0.0472;   // STL bbox x 0.5
    v->softener_radius = 0.65 * 0.0488;                                        // mushr_wheel.stl radius x (mushr_scale * 1.3) (:39,65-67)
}


void ftgp_tricycle_vehicle(FtgpVehicle* v)
{
    memset(v, 0, sizeof *v);
    v->kind = FTGP_VEHICLE_TRICYCLE;
    // masses: chassis mesh = convex hull of its 9 vertices at scale (0.01, 0.006, 0.0015), default density 1000 (car.em.xml:52,66): 0.4158
    // + LiDAR puck (density 2000, r 0.03, half-height 0.015; :78) 0.1696 + three wheels of 0.5 / 3 (:86,96,108,119)
    v->mass = 1.085446;
    v->izz = 0.005886;               // of those parts about the body origin
    v->wheel_x[0] = -0.07; v->wheel_y[0] = 0.06;      // left driven wheel (:97)
    v->wheel_x[1] = -0.07; v->wheel_y[1] = -0.06;     // right driven wheel (:110)
    v->wheel_x[2] = 0.08;  v->wheel_y[2] = 0.0;       // front caster: condim 1, frictionless (:96) -- carries load, transmits no force
    v->wheel_radius = 0.03;                           // cylinder size 0.03 0.01 (:24)
    v->wheel_inertia = 0.5 * (0.5 / 3.0) * 0.03 * 0.03;   // solid cylinder about its axle
    v->wheel_damping = 0.03;                          // default joint damping (:22)
    v->motor_forward_limit = 4.0; v->motor_turn_limit = 1.0;   // ctrlrange (:138-139)
    v->friction = 1.0; v->gravity = 9.81;             // MuJoCo default friction of wheel and plane
    v->tire_damping = (v->mass * (0.08 / 0.15) / 2.0) * (2.0 / (0.95 * 0.02));   // the load share of one driven wheel; solimp dmax 0.95 (:24), solref 0.02
    v->contact_x[0] = 0.045; v->contact_x[1] = 0.0; v->contact_x[2] = -0.045;    // chassis footprint 0.2 x 0.12 as three circles
    v->contact_radius = 0.06;
    v->contact_stiffness = v->mass / (0.95 * 0.95 * 0.02 * 0.02);
    v->contact_damping = v->mass * (2.0 / (0.95 * 0.02));
    v->lidar_x = -0.0525; v->lidar_y = 0.0; v->lidar_ring_radius = 0.03;         // (:72-76)
    v->body_z = 0.04;
    v->box_xmin = -0.10; v->box_xmax = 0.10; v->box_ymin = -0.06; v->box_ymax = 0.06;   // mesh bbox
    v->softener_radius = 0.035;                       // softener spheres (:93,104,116)
    v->steer_limit = 1.0; v->steer_inertia = 1.0;     // unused (no steering joint)
}

const char* ftgp_last_error(void) { return g_err; }

int ftgp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ftgp_destroy(FtgpEnv* e)
{
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream.get());
    if (e->side) (void)hipStreamSynchronize(e->side.get());
    if (e->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(e->comm);
    delete e;
    return 0;
}

int ftgp_create(const FtgpConfig* cfg, FtgpEnv** out)
{
    if (!cfg || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    *out = nullptr;
    const Switches sw = read_switches();
    if (int rc = validate(*cfg, &cfg->track, 1, false, sw)) return rc;
    return create(*cfg, &cfg->track, &cfg->n_envs, 1, sw, out);
}

int ftgp_create_tracks(const FtgpConfig* cfg, const FtgpTrack* tracks, const int32_t* envs_per_track, int n_tracks, FtgpEnv** out)
{
    if (!cfg || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    *out = nullptr;
    const Switches sw = read_switches();
    if (n_tracks < 1 || n_tracks > FTGP_MAX_TRACKS) return failf(FTGP_ERR_ARG, "ftgp_create_tracks: n_tracks = %d, not in 1 .. %d", n_tracks, FTGP_MAX_TRACKS);
    if (!tracks || !envs_per_track) return fail(FTGP_ERR_ARG, "ftgp_create_tracks: null tracks / envs_per_track%s");
    long long sum = 0;
    for (int k = 0; k < n_tracks; ++k) {
        if (envs_per_track[k] < 1) return failf(FTGP_ERR_ARG, "track %d: envs_per_track = %d, at least 1 env per track", k, (int)envs_per_track[k]);
        sum += envs_per_track[k];
    }
    if (sum != cfg->n_envs) return failf(FTGP_ERR_ARG, "ftgp_create_tracks: envs_per_track sums to %lld, n_envs is %d", sum, cfg->n_envs);
    if (int rc = validate(*cfg, tracks, n_tracks, true, sw)) return rc;
    return create(*cfg, tracks, envs_per_track, n_tracks, sw, out);
}

int ftgp_reset(FtgpEnv* e, const uint8_t* mask)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    e->rows_valid = false; e->launch_metrics_valid = false;
    HIP_TRY(hipSetDevice(e->device));
    const uint8_t* dmask = nullptr;
    if (mask) {
        HIP_TRY(hipMemcpyAsync(e->d_env_mask.get(), mask, (size_t)e->P.n_envs, hipMemcpyHostToDevice, e->stream.get()));
        dmask = e->d_env_mask.get();
    }
    hipLaunchKernelGGL(ftgp_reset_kernel, dim3((e->P.n_cars + 63) / 64), dim3(64), 0, e->stream.get(), e->P, dmask, (const int32_t*)e->d_env_track.get(), e->rule);
    HIP_TRY(hipGetLastError());
    if (e->rule) {      // every car has read its env's counter: the launch behind advances it
        hipLaunchKernelGGL(ftgp_episodes_kernel, dim3((e->P.n_envs + 63) / 64), dim3(64), 0, e->stream.get(), e->P.n_envs, dmask, e->d_episodes.get());
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ftgp_zero_ranges_kernel, dim3(e->P.n_cars), dim3(256), 0, e->stream.get(), e->P, dmask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_set_ctrl(FtgpEnv* e, const double* ctrl, const uint8_t* car_mask)
{
    if (!e || !ctrl) return fail(FTGP_ERR_ARG, "null argument%s");
    e->rows_valid = false;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(e->d_ctrl.get(), ctrl, sizeof(double) * 2 * (size_t)e->P.n_cars, hipMemcpyHostToDevice, e->stream.get()));
    const uint8_t* dmask = nullptr;
    if (car_mask) {
        HIP_TRY(hipMemcpyAsync(e->d_car_mask.get(), car_mask, (size_t)e->P.n_cars, hipMemcpyHostToDevice, e->stream.get()));
        dmask = e->d_car_mask.get();
    }
    hipLaunchKernelGGL(ftgp_set_ctrl_kernel, dim3((e->P.n_cars + 255) / 256), dim3(256), 0, e->stream.get(), e->P, e->d_ctrl.get(), dmask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream.get()));   // the caller's buffers may be reused as soon as we return
    return 0;
}

int ftgp_step(FtgpEnv* e, int n_steps)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    return launch_steps(e, FTGP_POLICY_HOST, n_steps);
}

int ftgp_rollout(FtgpEnv* e, int policy, int n_steps)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (policy < FTGP_POLICY_HOST || policy > FTGP_POLICY_NET3) return fail(FTGP_ERR_ARG, "unknown policy%s");
    return launch_steps(e, policy, n_steps);
}

int ftgp_set_car_policies(FtgpEnv* e, const int32_t* policies)
{
    if (!e || !policies) return fail(FTGP_ERR_ARG, "null argument%s");
    for (int k = 0; k < e->P.cars_per_env; ++k)
        if ((policies[k] < FTGP_POLICY_LOBOTOMY || policies[k] > FTGP_POLICY_RANDOM) && !is_net_policy(policies[k]))
            return fail(FTGP_ERR_ARG, "set_car_policies: lobotomy / nidc / fast / random / net0 .. net3 only%s");
    // a workgroup holds whole envs, so its car slot c runs the roster's entry c % cars_per_env
    for (int c = 0; c < FTGP_MAX_CARS_PER_BLOCK; ++c) e->P.car_policy[c] = policies[c % e->P.cars_per_env];
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the blocks while they change
    for (const TrackBufs& t : e->trk)     // every track's parameter block
        HIP_TRY(hipMemcpy(reinterpret_cast<unsigned char*>(e->d_params.get()) + t.block + offsetof(DeviceParams, car_policy), e->P.car_policy, sizeof e->P.car_policy, hipMemcpyHostToDevice));
    if (e->h_tables) memcpy(e->h_tables.get(), e->P.car_policy, sizeof e->P.car_policy);    // (no copy from it is pending: the stream is idle)
    e->table_on_device = 0;
    return 0;
}

int ftgp_device_io_config(FtgpEnv* e, const FtgpDeviceIoConfig* cfg)
{
    if (!e || !cfg) return fail(FTGP_ERR_ARG, "null argument%s");
    if (cfg->action_repeat < 1) return fail(FTGP_ERR_ARG, "device_io_config: action_repeat >= 1%s");
    const int cpe = e->P.cars_per_env;
    int32_t slot[FTGP_PAIR_STRIDE];
    int n_ext = 0; bool disparity = false;
    for (int k = 0; k < cpe; ++k) {
        slot[k] = cfg->roster ? cfg->roster[k] : FTGP_POLICY_HOST;
        if ((slot[k] < FTGP_POLICY_HOST || slot[k] > FTGP_POLICY_RANDOM) && !is_net_policy(slot[k]))
            return fail(FTGP_ERR_ARG, "device_io_config: host / lobotomy / nidc / fast / random / net0 .. net3 only%s");
        n_ext += slot[k] == FTGP_POLICY_HOST;
        disparity = disparity || slot[k] == FTGP_POLICY_NIDC || slot[k] == FTGP_POLICY_FAST;
    }
    if (n_ext == 0) return fail(FTGP_ERR_ARG, "device_io_config: at least one slot must be external (FTGP_POLICY_HOST)%s");
    if (disparity) if (int rc = check_disparity_shape(e->P)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no copy from the pinned tables is pending while they change
    if (!e->h_tables) {
        HIP_TRY(host_alloc(e->h_tables, sizeof(int32_t) * 2 * FTGP_MAX_CARS_PER_BLOCK, hipHostMallocDefault));
        memcpy(e->h_tables.get(), e->P.car_policy, sizeof e->P.car_policy);
        e->table_on_device = 0;
    }
    if (!e->ds.d_prev_abs) HIP_TRY(dev_alloc(e->ds.d_prev_abs, sizeof(int32_t) * (size_t)e->P.n_cars));
    // a workgroup holds whole envs, so its car slot c runs entry c % cars_per_env (as ftgp_set_car_policies)
    for (int c = 0; c < FTGP_MAX_CARS_PER_BLOCK; ++c) e->h_tables.get()[FTGP_MAX_CARS_PER_BLOCK + c] = slot[c % cpe];
    if (e->table_on_device == 1) e->table_on_device = -1;
    DeviceIoArgs& A = e->ds.io;
    A = DeviceIoArgs{};
    A.max_episode_steps = cfg->max_episode_steps; A.n_ext = n_ext; A.auto_reset = cfg->auto_reset ? 1 : 0;
    for (int k = 0, i = 0; k < FTGP_PAIR_STRIDE; ++k) A.ext_index[k] = (k < cpe && slot[k] == FTGP_POLICY_HOST) ? i++ : -1;
    A.prev_abs = e->ds.d_prev_abs.get();
    A.env_track = e->d_env_track.get();
    e->ds.repeat = cfg->action_repeat;
    e->ds.ready = true;
    set_signals(e, FtgpDeviceSignals{ 1, 0.0f, 0, 0.0f });
    e->ds.con_on = false;
    e->ds.frame_on = false;
    e->ds.rivals_on = false;
    return 0;
}

int ftgp_device_io_rivals(FtgpEnv* e, const FtgpDeviceRivals* rivals)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!e->ds.ready) return fail(FTGP_ERR_STATE, "ftgp_device_io_rivals before ftgp_device_io_config%s");
    if (!rivals) { e->ds.rivals_on = false; return 0; }
    if (rivals->n_rivals < 0 || rivals->n_rivals > FTGP_MAX_RIVALS) return fail(FTGP_ERR_ARG, "device_io_rivals: n_rivals in 0 .. 7%s");
    if (!nonneg_finite(rivals->place_weight)) return fail(FTGP_ERR_ARG, "device_io_rivals: place_weight >= 0 and finite%s");
    if (rivals->reserved != 0 || rivals->reserved_f != 0.0f) return fail(FTGP_ERR_ARG, "device_io_rivals: reserved fields must be 0%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_rival_rows(e)) return rc;
    e->ds.rivals = *rivals;
    e->ds.rivals_on = true;
    return 0;
}

int ftgp_device_io_frame(FtgpEnv* e, const FtgpDeviceFrame* frame)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!e->ds.ready) return fail(FTGP_ERR_STATE, "ftgp_device_io_frame before ftgp_device_io_config%s");
    if (!frame) { e->ds.frame_on = false; return 0; }
    if (frame->n_ahead < 0 || frame->n_ahead > FTGP_MAX_LOOKAHEAD) return fail(FTGP_ERR_ARG, "device_io_frame: n_ahead in 0 .. 16%s");
    if (frame->stride < 1 || frame->stride > FTGP_PATH_POINTS / 2) return fail(FTGP_ERR_ARG, "device_io_frame: stride in 1 .. 50%s");
    if (frame->reserved != 0) return fail(FTGP_ERR_ARG, "device_io_frame: reserved must be 0%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_frame_rows(e)) return rc;
    e->ds.frame = *frame;
    e->ds.frame_on = true;
    return 0;
}

int ftgp_device_io_contacts(FtgpEnv* e, const FtgpDeviceContacts* contacts)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!e->ds.ready) return fail(FTGP_ERR_STATE, "ftgp_device_io_contacts before ftgp_device_io_config%s");
    if (!contacts) { e->ds.con_on = false; return 0; }
    if (!nonneg_finite(contacts->wall_penalty)) return fail(FTGP_ERR_ARG, "device_io_contacts: wall_penalty >= 0 and finite%s");
    if (!nonneg_finite(contacts->car_penalty)) return fail(FTGP_ERR_ARG, "device_io_contacts: car_penalty >= 0 and finite%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_contact_rows(e)) return rc;
    e->ds.con = *contacts;
    e->ds.con_on = true;
    return 0;
}

int ftgp_device_io_signals(FtgpEnv* e, const FtgpDeviceSignals* signals)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!e->ds.ready) return fail(FTGP_ERR_STATE, "ftgp_device_io_signals before ftgp_device_io_config%s");
    const FtgpDeviceSignals s = signals ? *signals : FtgpDeviceSignals{ 1, 0.0f, 0, 0.0f };
    if (s.scan_pool < 1 || e->P.n_rays % s.scan_pool) return fail(FTGP_ERR_ARG, "device_io_signals: scan_pool >= 1 and a divisor of n_rays%s");
    if (!nonneg_finite(s.scan_max_range)) return fail(FTGP_ERR_ARG, "device_io_signals: scan_max_range >= 0 and finite%s");
    if (!nonneg_finite(s.off_track_penalty)) return fail(FTGP_ERR_ARG, "device_io_signals: off_track_penalty >= 0 and finite%s");
    set_signals(e, s);
    return 0;
}

int ftgp_step_device(FtgpEnv* e, const FtgpDeviceStep* io) { return ftgp_step_device_ex(e, io, nullptr); }

int ftgp_step_device_ex(FtgpEnv* e, const FtgpDeviceStep* io, const FtgpDeviceStepExtra* extra) { return ftgp_step_device_rivals(e, io, extra, nullptr, nullptr, nullptr); }

int ftgp_step_device_contacts(FtgpEnv* e, const FtgpDeviceStep* io, const FtgpDeviceStepExtra* extra, const FtgpDeviceStepContacts* contacts)
{
    return ftgp_step_device_rivals(e, io, extra, contacts, nullptr, nullptr);
}

int ftgp_step_device_frame(FtgpEnv* e, const FtgpDeviceStep* io, const FtgpDeviceStepExtra* extra, const FtgpDeviceStepContacts* contacts,
                           const FtgpDeviceStepFrame* frame)
{
    return ftgp_step_device_rivals(e, io, extra, contacts, frame, nullptr);
}

int ftgp_step_device_rivals(FtgpEnv* e, const FtgpDeviceStep* io, const FtgpDeviceStepExtra* extra, const FtgpDeviceStepContacts* contacts,
                            const FtgpDeviceStepFrame* frame, const FtgpDeviceStepRivals* rivals)
{
    DeviceStepPlan plan;
    if (int rc = plan_device_step(e, io, extra, contacts, frame, rivals, plan)) return rc;       // (before anything is enqueued)
    return on_handle_stream(e, io->stream, [&] { return enqueue_device_step(e, plan, [] { return 0; }); });
}

// LDS of a workgroup of ftgp_collect_act_kernel: four waves, each the rays its network's beams cover and the car's record
static size_t collect_act_lds(const NetDev& N) { return 4 * ((size_t)N.n_beams * (size_t)N.pool * sizeof(float) + sizeof(CarCore)); }

// ftgp_collect_act_kernel on the handle's stream for the rows of one decision: inputs, mean and action -- or, with mean == null, the
// inputs alone (next_inputs)
// (value != null: the VALUE instantiations, which also evaluate the slot's value net into value -- ftgp_collect_values_device)
static int launch_collect_act(FtgpEnv* e, const FtgpCollect& c, const float* noise, float* inputs, float* mean, float* action, float* value = nullptr)
{
    CollectValueArgs C{};
    C.noise = noise; C.inputs = inputs; C.mean = mean; C.action = action;
    for (int k = 0; k < 2; ++k) { C.std[k] = c.std[k]; C.lo[k] = c.lo[k]; C.hi[k] = c.hi[k]; }
    C.slot = c.slot; C.n_ext = e->ds.io.n_ext; C.n_rows = e->P.n_envs * e->ds.io.n_ext;
    for (int k = 0; k < FTGP_PAIR_STRIDE; ++k) if (e->ds.io.ext_index[k] >= 0) C.ext_slot[e->ds.io.ext_index[k]] = k;
    C.env_track = e->d_env_track.get();
    const size_t lds = collect_act_lds(e->slots[c.slot].net);
    if (value) {
        C.vnet = e->d_vnets.get() + c.slot; C.value = value;
        void (*kernel)(DeviceParams, CollectValueArgs) = mean ? ftgp_collect_act_kernel<true, true> : ftgp_collect_act_kernel<false, true>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((C.n_rows + 3) / 4)), dim3(256), lds, e->stream.get(), e->P, C);
    } else {
        void (*kernel)(DeviceParams, CollectActArgs) = mean ? ftgp_collect_act_kernel<true> : ftgp_collect_act_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((C.n_rows + 3) / 4)), dim3(256), lds, e->stream.get(), e->P, static_cast<const CollectActArgs&>(C));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// gamma and lam of ftgp_collect_values_device and ftgp_gae_device: finite, in [0, 1]
static int check_discount(const char* entry, const char* name, float v)
{
    if (!std::isfinite(v) || v < 0.0f || v > 1.0f) return failf(FTGP_ERR_ARG, "%s: %s = %g must be finite and in [0, 1]", entry, name, (double)v);
    return 0;
}

// ftgp_gae_kernel on the handle's stream: the advantage scan over T decisions of the handle's external rows (the buffers are checked)
static int launch_gae(FtgpEnv* e, size_t T, float gamma, float lam, const float* reward, const float* value, const float* next_value,
                      const uint8_t* terminated, const uint8_t* truncated, float* advantage, float* ret)
{
    GaeArgs G{};
    G.reward = reward; G.value = value; G.next_value = next_value; G.terminated = terminated; G.truncated = truncated;
    G.advantage = advantage; G.ret = ret;
    G.gamma = gamma; G.gl = gamma * lam;
    G.T = (int32_t)T; G.n_ext = e->ds.io.n_ext; G.n_envs = e->P.n_envs; G.n_rows = e->P.n_envs * e->ds.io.n_ext;
    hipLaunchKernelGGL(ftgp_gae_kernel, dim3((unsigned)((G.n_rows + 255) / 256)), dim3(256), 0, e->stream.get(), G);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ftgp_collect_device(FtgpEnv* e, const FtgpCollect* c) { return ftgp_collect_values_device(e, c, nullptr); }

int ftgp_collect_values_device(FtgpEnv* e, const FtgpCollect* c, const FtgpCollectValues* v)
{
    if (!e || !c) return fail(FTGP_ERR_ARG, "null argument%s");
    FtgpEnv::DeviceStep& ds = e->ds;
    if (!ds.ready) return fail(FTGP_ERR_STATE, "ftgp_collect_device before ftgp_device_io_config%s");
    if (c->reserved != 0) return fail(FTGP_ERR_ARG, "ftgp_collect_device: reserved must be 0%s");
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_collect_device", c->slot, kSlotDefined, S)) return rc;
    if (c->n_decisions < 1) return failf(FTGP_ERR_ARG, "ftgp_collect_device: n_decisions = %d must be >= 1", c->n_decisions);
    for (int k = 0; k < 2; ++k) {
        if (!nonneg_finite(c->std[k])) return failf(FTGP_ERR_ARG, "ftgp_collect_device: std[%d] = %g must be >= 0 and finite", k, (double)c->std[k]);
        if (!std::isfinite(c->lo[k])) return failf(FTGP_ERR_ARG, "ftgp_collect_device: lo[%d] is not finite", k);
        if (!std::isfinite(c->hi[k])) return failf(FTGP_ERR_ARG, "ftgp_collect_device: hi[%d] is not finite", k);
        if (!(c->lo[k] <= c->hi[k])) return failf(FTGP_ERR_ARG, "ftgp_collect_device: lo[%d] = %g above hi[%d] = %g", k, (double)c->lo[k], k, (double)c->hi[k]);
    }
    // (a FTGP_LIDAR_FAKELIDAR handle, where ftgp_set_dynamics is FTGP_ERR_STATE, has no defined slot: ftgp_set_net refuses it)
    if (c->reset_dynamics && !ds.io.auto_reset) return fail(FTGP_ERR_STATE, "ftgp_collect_device: reset_dynamics while auto_reset is off (ftgp_device_io_config)%s");
    if (collect_act_lds(S->net) > 64 * 1024)
        return failf(FTGP_ERR_ARG, "ftgp_collect_device: slot %d: the %d rays of its beams (n_beams * pool) do not fit LDS four cars to a workgroup", c->slot, S->net.n_beams * S->net.pool);
    HIP_TRY(hipSetDevice(e->device));
    // every buffer at its full T-fold size
    const size_t T = (size_t)c->n_decisions, n_envs = (size_t)e->P.n_envs, rows = n_envs * (size_t)ds.io.n_ext, n_in = (size_t)S->net.width[0];
    auto checked = [&](const void* p, size_t per_decision, const char* name) { return check_device_buffer(e, "ftgp_collect_device", p, T, per_decision, name); };
    if (c->noise) if (int rc = checked(c->noise, sizeof(float) * 2 * rows, "noise")) return rc;
    if (int rc = checked(c->inputs, sizeof(float) * n_in * rows, "inputs")) return rc;
    if (int rc = checked(c->mean, sizeof(float) * 2 * rows, "mean")) return rc;
    if (int rc = checked(c->action, sizeof(float) * 2 * rows, "action")) return rc;
    if (int rc = checked(c->reward, sizeof(float) * rows, "reward")) return rc;
    if (int rc = checked(c->terminated, n_envs, "terminated")) return rc;
    if (int rc = checked(c->truncated, n_envs, "truncated")) return rc;
    if (c->next_inputs) if (int rc = checked(c->next_inputs, sizeof(float) * n_in * rows, "next_inputs")) return rc;
    if (c->reset_dynamics) if (int rc = checked(c->reset_dynamics, sizeof(double) * FTGP_DYN_DOUBLES * (size_t)e->P.n_cars, "reset_dynamics")) return rc;
    if (v) {
        auto checked_v = [&](const void* p, const char* name) { return check_device_buffer(e, "ftgp_collect_values_device", p, T, sizeof(float) * rows, name); };
        if (int rc = net_slot(e, "ftgp_collect_values_device", c->slot, kSlotValue, S)) return rc;
        if (v->reserved[0] != 0 || v->reserved[1] != 0) return fail(FTGP_ERR_ARG, "ftgp_collect_values_device: reserved must be 0%s");
        if (int rc = check_discount("ftgp_collect_values_device", "gamma", v->gamma)) return rc;
        if (int rc = check_discount("ftgp_collect_values_device", "lam", v->lam)) return rc;
        if ((v->advantage == nullptr) != (v->ret == nullptr))
            return failf(FTGP_ERR_ARG, "ftgp_collect_values_device: %s is given without %s (both or neither)", v->advantage ? "advantage" : "ret", v->advantage ? "ret" : "advantage");
        if (int rc = checked_v(v->value, "value")) return rc;
        if (int rc = checked_v(v->next_value, "next_value")) return rc;
        if (v->advantage) {
            if (int rc = checked_v(v->advantage, "advantage")) return rc;
            if (int rc = checked_v(v->ret, "ret")) return rc;
        }
    }
    // the obs rows of the device step are not part of the record: scratch of the handle's, at the widest row a signals setting gives
    if (!ds.d_collect_obs) HIP_TRY(dev_alloc(ds.d_collect_obs, sizeof(float) * (size_t)e->P.n_cars * (size_t)e->P.n_rays));
    const FtgpDeviceStep io{ c->stream, c->action, ds.d_collect_obs.get(), c->reward, c->terminated, c->truncated, nullptr };
    DeviceStepPlan plan;
    if (int rc = plan_device_step(e, &io, nullptr, nullptr, nullptr, nullptr, plan)) return rc;
    if (c->reset_dynamics) if (int rc = ensure_dynamics(e)) return rc;
    return on_handle_stream(e, c->stream, [&] {
        for (size_t t = 0; t < T; ++t) {
            float* action = c->action + t * rows * 2;
            if (int rc = launch_collect_act(e, *c, c->noise ? c->noise + t * rows * 2 : nullptr, c->inputs + t * rows * n_in, c->mean + t * rows * 2, action,
                                            v ? v->value + t * rows : nullptr)) return rc;
            plan.A.action = action; plan.A.reward = c->reward + t * rows; plan.A.terminated = c->terminated + t * n_envs; plan.A.truncated = c->truncated + t * n_envs;
            // (step 3': with a value net the kernel runs whether or not next_inputs is given, and writes x down only where it is)
            if (int rc = enqueue_device_step(e, plan, [&] {
                    if (v) return launch_collect_act(e, *c, nullptr, c->next_inputs ? c->next_inputs + t * rows * n_in : nullptr, nullptr, nullptr, v->next_value + t * rows);
                    return c->next_inputs ? launch_collect_act(e, *c, nullptr, c->next_inputs + t * rows * n_in, nullptr, nullptr) : 0; })) return rc;
            if (c->reset_dynamics)
                if (int rc = launch_dynamics(e, c->reset_dynamics + t * (size_t)e->P.n_cars * FTGP_DYN_DOUBLES, plan.A.terminated, plan.A.truncated)) return rc;
        }
        if (v && v->advantage)
            if (int rc = launch_gae(e, T, v->gamma, v->lam, c->reward, v->value, v->next_value, c->terminated, c->truncated, v->advantage, v->ret)) return rc;
        return 0;
    });
}

int ftgp_gae_device(FtgpEnv* e, void* stream, int n_decisions, float gamma, float lam, const float* reward, const float* value, const float* next_value,
                    const uint8_t* terminated, const uint8_t* truncated, float* advantage, float* ret)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!e->ds.ready) return fail(FTGP_ERR_STATE, "ftgp_gae_device before ftgp_device_io_config%s");
    if (n_decisions < 1) return failf(FTGP_ERR_ARG, "ftgp_gae_device: n_decisions = %d must be >= 1", n_decisions);
    if (int rc = check_discount("ftgp_gae_device", "gamma", gamma)) return rc;
    if (int rc = check_discount("ftgp_gae_device", "lam", lam)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t T = (size_t)n_decisions, n_envs = (size_t)e->P.n_envs, rows = n_envs * (size_t)e->ds.io.n_ext;
    auto checked = [&](const void* p, size_t per_decision, const char* name) { return check_device_buffer(e, "ftgp_gae_device", p, T, per_decision, name); };
    if (int rc = checked(reward, sizeof(float) * rows, "reward")) return rc;
    if (int rc = checked(value, sizeof(float) * rows, "value")) return rc;
    if (int rc = checked(next_value, sizeof(float) * rows, "next_value")) return rc;
    if (int rc = checked(terminated, n_envs, "terminated")) return rc;
    if (int rc = checked(truncated, n_envs, "truncated")) return rc;
    if (int rc = checked(advantage, sizeof(float) * rows, "advantage")) return rc;
    if (int rc = checked(ret, sizeof(float) * rows, "ret")) return rc;
    return on_handle_stream(e, stream, [&] { return launch_gae(e, T, gamma, lam, reward, value, next_value, terminated, truncated, advantage, ret); });
}

int ftgp_state_device(FtgpEnv* e, void* stream, float* state)
{
    return rows_to_device(e, "ftgp_state_device", stream, FTGP_STATE_FLOATS, state, "state", [&] {
        hipLaunchKernelGGL(ftgp_io_state_kernel, dim3((unsigned)((e->P.n_cars + 255) / 256)), dim3(256), 0, e->stream.get(), e->P, e->ds.io, state);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int ftgp_contacts_device(FtgpEnv* e, void* stream, float* contact)
{
    return rows_to_device(e, "ftgp_contacts_device", stream, FTGP_CONTACT_FLOATS, contact, "contact", [&] { return launch_contacts(e, nullptr, contact); });
}

int ftgp_frame_device(FtgpEnv* e, void* stream, float* frame)
{
    const bool on = e && e->ds.frame_on;
    const int n_ahead = on ? e->ds.frame.n_ahead : 0, stride = on ? e->ds.frame.stride : 1;
    return rows_to_device(e, "ftgp_frame_device", stream, (size_t)(FTGP_FRAME_FIXED + 2 * n_ahead), frame, "frame", [&] { return launch_frame(e, n_ahead, stride, nullptr, frame, -1); });
}

int ftgp_rivals_device(FtgpEnv* e, void* stream, float* rival)
{
    const int n_rivals = e && e->ds.rivals_on ? e->ds.rivals.n_rivals : 0;
    return rows_to_device(e, "ftgp_rivals_device", stream, (size_t)(FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * n_rivals), rival, "rival", [&] {
        if (int rc = ensure_rival_rows(e)) return rc;
        return launch_rivals_now(e, n_rivals, nullptr, rival);
    });
}

int ftgp_set_spawn_rule(FtgpEnv* e, const FtgpSpawnRule* r)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    const size_t T = (size_t)e->n_tracks, n_envs = (size_t)e->P.n_envs;
    std::vector<int32_t> start(FTGP_PATH_POINTS * T, 0), n_start(T, 0);
    std::vector<double> clear(2 * FTGP_PATH_POINTS * T, 0.0);
    if (r) {
        if (r->first_point < 0 || r->first_point >= FTGP_PATH_POINTS) return fail(FTGP_ERR_ARG, "set_spawn_rule: first_point in 0 .. 99%s");
        if (r->n_points < 1 || r->n_points > FTGP_PATH_POINTS) return fail(FTGP_ERR_ARG, "set_spawn_rule: n_points in 1 .. 100%s");
        if (r->reserved != 0) return fail(FTGP_ERR_ARG, "set_spawn_rule: reserved must be 0%s");
        if (!nonneg_finite(r->margin)) return fail(FTGP_ERR_ARG, "set_spawn_rule: margin >= 0 and finite%s");
        if (!(r->lateral_frac >= 0.0 && r->lateral_frac <= 1.0)) return fail(FTGP_ERR_ARG, "set_spawn_rule: lateral_frac in [0, 1]%s");
        if (!nonneg_finite(r->yaw_tan)) return fail(FTGP_ERR_ARG, "set_spawn_rule: yaw_tan >= 0 and finite%s");
        for (size_t k = 0; k < T; ++k) {
            for (int p = 0; p < FTGP_PATH_POINTS; ++p) memcpy(&clear[2 * (FTGP_PATH_POINTS * k + p)], &e->start_table[6 * (FTGP_PATH_POINTS * k + p) + 4], sizeof(double) * 2);
            n_start[k] = ftgp_start_list(*r, &clear[2 * FTGP_PATH_POINTS * k], &start[FTGP_PATH_POINTS * k]);
            if (n_start[k] == 0)
                return failf(FTGP_ERR_ARG, "track %d: set_spawn_rule: none of the %d points from %d on keeps %g of clearance on both sides", (int)k, r->n_points, r->first_point, r->margin);
        }
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the tables or the counters while they change
    if (r) {
        if (!e->d_start) HIP_TRY(dev_alloc(e->d_start, sizeof(int32_t) * start.size()));
        if (!e->d_n_start) HIP_TRY(dev_alloc(e->d_n_start, sizeof(int32_t) * n_start.size()));
        if (!e->d_clear) HIP_TRY(dev_alloc(e->d_clear, sizeof(double) * clear.size()));
        if (!e->d_episodes) HIP_TRY(dev_alloc(e->d_episodes, sizeof(int64_t) * n_envs));
        if (!e->d_rule) HIP_TRY(dev_alloc(e->d_rule, sizeof(FtgpSpawnDev)));
        FtgpSpawnDev d{};
        d.start = e->d_start.get(); d.n_start = e->d_n_start.get(); d.clear = e->d_clear.get(); d.episodes = e->d_episodes.get();
        d.margin = r->margin; d.lateral_frac = r->lateral_frac; d.yaw_tan = r->yaw_tan; d.shuffle_grid = r->shuffle_grid ? 1 : 0;
        HIP_TRY(hipMemcpy(e->d_rule.get(), &d, sizeof d, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_start.get(), start.data(), sizeof(int32_t) * start.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_n_start.get(), n_start.data(), sizeof(int32_t) * n_start.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_clear.get(), clear.data(), sizeof(double) * clear.size(), hipMemcpyHostToDevice));
    }
    if (e->d_episodes) {
        HIP_TRY(hipMemsetAsync(e->d_episodes.get(), 0, sizeof(int64_t) * n_envs, e->stream.get()));
        HIP_TRY(hipStreamSynchronize(e->stream.get()));
    }
    e->rule = r ? e->d_rule.get() : nullptr;
    return 0;
}

int ftgp_set_dynamics(FtgpEnv* e, const double* rows, const uint8_t* env_mask)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (e->P.lidar_mode == FTGP_LIDAR_FAKELIDAR) return fail(FTGP_ERR_STATE, "ftgp_set_dynamics: not on a FTGP_LIDAR_FAKELIDAR handle%s");
    const size_t n_cars = (size_t)e->P.n_cars;
    HIP_TRY(hipSetDevice(e->device));
    if (!rows) {                     // off: later launches run the kernels of a handle without a table
        if (env_mask) return fail(FTGP_ERR_ARG, "ftgp_set_dynamics: a mask without rows%s");
        if (e->d_dyn) HIP_TRY(hipMemsetAsync(dyn_rejected(&e->P), 0, sizeof(unsigned long long), e->stream.get()));
        HIP_TRY(hipStreamSynchronize(e->stream.get()));
        e->dyn_on = false;
        return 0;
    }
    static const char* const names[FTGP_DYN_DOUBLES] = { "mass", "izz", "friction", "tire_damping", "throttle_kv", "throttle_force_limit", "steer_kp", "steer_damping" };
    for (size_t i = 0; i < n_cars; ++i) {
        if (env_mask && !env_mask[i / (size_t)e->P.cars_per_env]) continue;
        for (int k = 0; k < FTGP_DYN_DOUBLES; ++k) {
            const double x = rows[i * FTGP_DYN_DOUBLES + k];
            if (!(k < 2 ? x > 0.0 : x >= 0.0) || std::isinf(x))
                return failf(FTGP_ERR_ARG, "ftgp_set_dynamics: car %zu, entry %d (%s) = %g: every entry finite, mass and izz > 0, the others >= 0", i, k, names[k], x);
        }
    }
    if (!e->d_dyn_rows) HIP_TRY(dev_alloc(e->d_dyn_rows, sizeof(double) * FTGP_DYN_DOUBLES * n_cars));
    HIP_TRY(hipMemcpyAsync(e->d_dyn_rows.get(), rows, sizeof(double) * FTGP_DYN_DOUBLES * n_cars, hipMemcpyHostToDevice, e->stream.get()));
    const uint8_t* dmask = nullptr;
    if (env_mask) {
        HIP_TRY(hipMemcpyAsync(e->d_env_mask.get(), env_mask, (size_t)e->P.n_envs, hipMemcpyHostToDevice, e->stream.get()));
        dmask = e->d_env_mask.get();
    }
    if (int rc = launch_dynamics(e, e->d_dyn_rows.get(), dmask)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream.get()));   // the caller's buffers may be reused as soon as we return
    return 0;
}

int ftgp_set_dynamics_device(FtgpEnv* e, void* stream, const double* rows, const uint8_t* env_mask)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (e->P.lidar_mode == FTGP_LIDAR_FAKELIDAR) return fail(FTGP_ERR_STATE, "ftgp_set_dynamics_device: not on a FTGP_LIDAR_FAKELIDAR handle%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = check_device_buffer(e, "ftgp_set_dynamics_device", rows, sizeof(double) * FTGP_DYN_DOUBLES * (size_t)e->P.n_cars, "rows")) return rc;
    if (env_mask) if (int rc = check_device_buffer(e, "ftgp_set_dynamics_device", env_mask, (size_t)e->P.n_envs, "env_mask")) return rc;
    return on_handle_stream(e, stream, [&] { return launch_dynamics(e, rows, env_mask); });
}

int ftgp_get_dynamics(FtgpEnv* e, double* rows_out, int64_t* rejected_out)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    const size_t n_cars = (size_t)e->P.n_cars;
    if (!e->dyn_on) {
        if (rows_out) for (size_t i = 0; i < n_cars; ++i) memcpy(rows_out + i * FTGP_DYN_DOUBLES, e->dyn.base, sizeof e->dyn.base);
        if (rejected_out) *rejected_out = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(e->device));
    unsigned long long rejected = 0;
    if (rows_out)        // the first eight doubles of every record
        HIP_TRY(hipMemcpy2DAsync(rows_out, sizeof(double) * FTGP_DYN_DOUBLES, dyn_table(&e->P), sizeof(double) * FTGP_DYN_RECORD,
                                 sizeof(double) * FTGP_DYN_DOUBLES, n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipMemcpyAsync(&rejected, dyn_rejected(&e->P), sizeof rejected, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    if (rejected_out) *rejected_out = (int64_t)rejected;
    return 0;
}

// ---- network drivers ----
// What the description of a policy and of a value net share (`entry`: the setter in the message): n_layers, width[] with `last` outputs on the
// last layer, the two activations.
static int check_layers(const char* entry, int last, int n_layers, const int32_t* width, int hidden_act, int out_act)
{
    if (n_layers < 1 || n_layers > FTGP_NET_MAX_LAYERS) return failf(FTGP_ERR_ARG, "%s: n_layers = %d outside 1 .. %d", entry, n_layers, FTGP_NET_MAX_LAYERS);
    for (int l = 0; l < FTGP_NET_MAX_LAYERS; ++l) {
        const int w = width[l];
        if (l >= n_layers) { if (w != 0) return failf(FTGP_ERR_ARG, "%s: width[%d] = %d behind the last layer must be 0", entry, l, w); }
        else if (l == n_layers - 1) { if (w != last) return failf(FTGP_ERR_ARG, "%s: width[%d] = %d: the last layer has exactly %d output%s", entry, l, w, last, last == 1 ? "" : "s"); }
        else if (w < 1 || w > FTGP_NET_MAX_HIDDEN) return failf(FTGP_ERR_ARG, "%s: width[%d] = %d outside 1 .. %d", entry, l, w, FTGP_NET_MAX_HIDDEN);
    }
    if (hidden_act < FTGP_ACT_IDENTITY || hidden_act > FTGP_ACT_TANH) return failf(FTGP_ERR_ARG, "%s: hidden_act = %d is no FTGP_ACT_*", entry, hidden_act);
    if (out_act < FTGP_ACT_IDENTITY || out_act > FTGP_ACT_TANH) return failf(FTGP_ERR_ARG, "%s: out_act = %d is no FTGP_ACT_*", entry, out_act);
    return 0;
}

// what ftgp_set_net checks of a description on a handle of R rays whose drivers read rays [eighth, R - eighth) (include/ftgp.h); the message
// names the field
static int check_net_desc(int R, int eighth, const FtgpNetDesc& d)
{
    if (d.reserved != 0) return fail(FTGP_ERR_ARG, "ftgp_set_net: reserved must be 0%s");
    if (d.pool < 1 || R % d.pool != 0) return failf(FTGP_ERR_ARG, "ftgp_set_net: pool = %d must be >= 1 and divide n_rays = %d", d.pool, R);
    if (!(d.max_range > 0.0f) || std::isinf(d.max_range)) return failf(FTGP_ERR_ARG, "ftgp_set_net: max_range = %g must be finite and > 0", (double)d.max_range);
    if (d.n_beams < 1 || d.beam_first < 0 || d.n_beams > FTGP_NET_MAX_INPUTS || d.beam_first > R)
        return failf(FTGP_ERR_ARG, "ftgp_set_net: beam_first = %d, n_beams = %d out of range", d.beam_first, d.n_beams);
    if ((int64_t)d.beam_first * d.pool < eighth || (int64_t)(d.beam_first + d.n_beams) * d.pool > R - eighth)
        return failf(FTGP_ERR_ARG, "ftgp_set_net: beams %d .. %d of pool %d leave the drivers' scan window, rays [%d, %d) of %d (beam_first, n_beams)", d.beam_first,
                     d.beam_first + d.n_beams - 1, d.pool, eighth, R - eighth, R);
    if (d.use_state != 0 && d.use_state != 1) return failf(FTGP_ERR_ARG, "ftgp_set_net: use_state = %d must be 0 or 1", d.use_state);
    // (the input width has always been looked at behind n_layers and before width[]: a description wrong in two ways keeps its message)
    const bool count_ok = d.n_layers >= 1 && d.n_layers <= FTGP_NET_MAX_LAYERS;
    if (count_ok && ftgp_net_inputs(&d) > FTGP_NET_MAX_INPUTS) return failf(FTGP_ERR_ARG, "ftgp_set_net: n_beams + 5 use_state = %d inputs, at most %d", ftgp_net_inputs(&d), FTGP_NET_MAX_INPUTS);
    if (int rc = check_layers("ftgp_set_net", 2, d.n_layers, d.width, d.hidden_act, d.out_act)) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(d.out_scale[k])) return failf(FTGP_ERR_ARG, "ftgp_set_net: out_scale[%d] is not finite", k);
        if (!std::isfinite(d.out_offset[k])) return failf(FTGP_ERR_ARG, "ftgp_set_net: out_offset[%d] is not finite", k);
    }
    return 0;
}

// what ftgp_set_net_frame checks beyond the description: the frame struct (as ftgp_device_io_frame checks its own: the ranges hold
// for a struct that is off too) and the width with the frame entries
static int check_net_frame(const FtgpNetDesc& d, const FtgpNetFrame& f)
{
    if (f.enabled != 0 && f.enabled != 1) return failf(FTGP_ERR_ARG, "ftgp_set_net_frame: enabled = %d must be 0 or 1", f.enabled);
    if (f.n_ahead < 0 || f.n_ahead > FTGP_MAX_LOOKAHEAD) return failf(FTGP_ERR_ARG, "ftgp_set_net_frame: n_ahead = %d outside 0 .. %d", f.n_ahead, FTGP_MAX_LOOKAHEAD);
    if (f.stride < 1 || f.stride > 50) return failf(FTGP_ERR_ARG, "ftgp_set_net_frame: stride = %d outside 1 .. 50", f.stride);
    if (f.reserved != 0) return fail(FTGP_ERR_ARG, "ftgp_set_net_frame: reserved must be 0%s");
    const int n_in = ftgp_net_inputs(&d) + ftgp_net_frame_inputs(&f);
    if (n_in > FTGP_NET_MAX_INPUTS)
        return failf(FTGP_ERR_ARG, "ftgp_set_net_frame: n_in = n_beams + 5 use_state + %d frame entries = %d inputs, at most %d", ftgp_net_frame_inputs(&f), n_in, FTGP_NET_MAX_INPUTS);
    return 0;
}

// what ftgp_set_net_rivals checks beyond that: the rivals struct (n_rivals holds for a struct that is off too) and the width with the
// rival entries behind the frame's
static int check_net_rivals(const FtgpNetDesc& d, const FtgpNetFrame* f, const FtgpNetRivals& r)
{
    if (r.enabled != 0 && r.enabled != 1) return failf(FTGP_ERR_ARG, "ftgp_set_net_rivals: enabled = %d must be 0 or 1", r.enabled);
    if (r.n_rivals < 0 || r.n_rivals > FTGP_MAX_RIVALS) return failf(FTGP_ERR_ARG, "ftgp_set_net_rivals: n_rivals = %d outside 0 .. %d", r.n_rivals, FTGP_MAX_RIVALS);
    if (r.reserved[0] != 0 || r.reserved[1] != 0) return fail(FTGP_ERR_ARG, "ftgp_set_net_rivals: reserved must be 0%s");
    const int n_in = ftgp_net_inputs(&d) + ftgp_net_frame_inputs(f) + ftgp_net_rival_inputs(&r);
    if (n_in > FTGP_NET_MAX_INPUTS)
        return failf(FTGP_ERR_ARG, "ftgp_set_net_rivals: n_in = n_beams + 5 use_state + %d frame entries + %d rival entries = %d inputs, at most %d",
                     ftgp_net_frame_inputs(f), ftgp_net_rival_inputs(&r), n_in, FTGP_NET_MAX_INPUTS);
    return 0;
}

// floats of a record's parameters in the caller's layout: per layer W[n_out][n_in], then b[n_out], with the slot's true n_in
static size_t net_param_count(const NetDev& N)
{
    size_t n = 0;
    for (int l = 0; l < N.n_layers; ++l) n += (size_t)N.width[l + 1] * (size_t)N.width[l] + (size_t)N.width[l + 1];
    return n;
}

// the layers of a record in the library's layout: n_in inputs, then width[l] outputs of layer l; where Wt and b of each layer sit, and
// the floats of the whole set
static void lay_out_layers(NetDev& N, int n_in, int n_layers, const int32_t* width)
{
    N.n_layers = n_layers; N.width[0] = n_in;
    int o = 0;
    for (int l = 0; l < n_layers; ++l) {
        N.width[l + 1] = width[l];
        const int ld = (width[l] + FTGP_WAVE - 1) & ~(FTGP_WAVE - 1);
        N.w_off[l] = o; o += N.width[l] * ld;
        N.b_off[l] = o; o += ld;
    }
    N.n_floats = o;
}

// the record of a description: the library's layout (NetDev) without the buffer's address; f = null: no frame inputs, r = null: no rival inputs
static NetDev net_record(const FtgpNetDesc& d, const FtgpNetFrame* f, const FtgpNetRivals* r)
{
    NetDev N{};
    N.defined = 1; N.pool = d.pool; N.beam_first = d.beam_first; N.n_beams = d.n_beams; N.use_state = d.use_state;
    N.hidden_act = d.hidden_act; N.out_act = d.out_act;
    if (f && f->enabled) { N.frame_first = ftgp_net_inputs(&d); N.frame_shape = f->n_ahead | f->stride << 8; }
    if (r && r->enabled) { N.rival_first = ftgp_net_inputs(&d) + ftgp_net_frame_inputs(f); N.rival_shape = 1 | r->n_rivals << 8; }
    lay_out_layers(N, ftgp_net_inputs(&d) + ftgp_net_frame_inputs(f) + ftgp_net_rival_inputs(r), d.n_layers, d.width);
    N.max_range = d.max_range; N.inv_max_range = 1.0f / d.max_range;
    for (int k = 0; k < 2; ++k) { N.out_scale[k] = d.out_scale[k]; N.out_offset[k] = d.out_offset[k]; }
    return N;
}

// a host buffer of n elements for a network entry: a failed allocation is an error code, no exception crosses the C interface
extern "C++" {
template <class T> static int net_host_buffer(std::vector<T>& v, size_t n, const char* entry)
{
    try { v.assign(n, T()); }
    catch (const std::bad_alloc&) { return failf(FTGP_ERR_HIP, "%s: no host memory for %zu bytes", entry, n * sizeof(T)); }
    return 0;
}
}

// The three ways of a parameter set of record N's shape between a caller and the library's layout.
// in from the host: n_members sets in the caller's layout (a slot's single set: 1) -> the library's layout, `floats` floats with the padding
// zeros -> a new device buffer
static int upload_params(const char* entry, const NetDev& N, int n_members, size_t floats, const float* params, DevBuf<float>& buf)
{
    std::vector<float> img;
    if (int rc = net_host_buffer(img, floats, entry)) return rc;
    ftgp_net_population_to_library(N.n_layers, N.width, n_members, params, img.data());
    HIP_TRY(dev_upload(buf, img.data(), sizeof(float) * img.size()));
    return 0;
}
// out to the host: one set in the library's layout at `src` on the device -> the caller's layout; the handle's stream is synchronised
static int download_params(FtgpEnv* e, const char* entry, const NetDev& N, const float* src, float* out)
{
    std::vector<float> img;
    if (int rc = net_host_buffer(img, (size_t)N.n_floats, entry)) return rc;
    HIP_TRY(hipMemcpyAsync(img.data(), src, sizeof(float) * img.size(), hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    ftgp_net_population_from_library(N.n_layers, N.width, 1, img.data(), out);
    return 0;
}
// in from the device: ftgp_net_params_kernel on the handle's stream, n_members sets of a caller's device buffer in the caller's layout -> the
// library's layout at dst, `stride` floats apart (a slot's single set: 1 member, stride 0)
static int launch_net_params(FtgpEnv* e, const NetDev& N, const float* params, float* dst, int stride, int n_members)
{
    const int n = (int)net_param_count(N);
    hipLaunchKernelGGL(ftgp_net_params_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min(n_members, FTGP_NET_PARAMS_GRID_Y)), dim3(256), 0, e->stream.get(), N, params,
                       dst, n, stride, n_members);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The first setter call of a handle: the NET kernels may use the LDS the others may, the records are allocated (zeroed: every slot
// empty) and every parameter block learns their address.  ftgp_create does nothing for the networks.
static int ensure_nets(FtgpEnv* e)
{
    if (e->d_nets) return 0;
    for (const auto& set : kStepKernelsNet) for (const auto& row : set) for (const StepKernel& k : row) HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the blocks while they change
    DevBuf<NetDev> d;
    HIP_TRY(dev_alloc(d, sizeof(NetDev) * FTGP_MAX_NETS));
    HIP_TRY(hipMemset(d.get(), 0, sizeof(NetDev) * FTGP_MAX_NETS));
    const uint64_t a = (uint64_t)(uintptr_t)d.get();
    const uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
    for (const TrackBufs& t : e->trk) {   // every track's parameter block
        unsigned char* block = reinterpret_cast<unsigned char*>(e->d_params.get()) + t.block;
        HIP_TRY(hipMemcpy(block + offsetof(DeviceParams, net_table_lo), &lo, sizeof lo, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(block + offsetof(DeviceParams, net_table_hi), &hi, sizeof hi, hipMemcpyHostToDevice));
    }
    e->P.net_table_lo = lo; e->P.net_table_hi = hi;
    e->d_nets = std::move(d);
    return 0;
}

int ftgp_set_net(FtgpEnv* e, int slot, const FtgpNetDesc* desc, const float* params) { return ftgp_set_net_rivals(e, slot, desc, nullptr, nullptr, params); }

int ftgp_set_net_frame(FtgpEnv* e, int slot, const FtgpNetDesc* desc, const FtgpNetFrame* frame, const float* params) { return ftgp_set_net_rivals(e, slot, desc, frame, nullptr, params); }

int ftgp_set_net_rivals(FtgpEnv* e, int slot, const FtgpNetDesc* desc, const FtgpNetFrame* frame, const FtgpNetRivals* rivals, const float* params)
{
    if (e && e->P.lidar_mode == FTGP_LIDAR_FAKELIDAR) return fail(FTGP_ERR_STATE, "ftgp_set_net: not on a FTGP_LIDAR_FAKELIDAR handle%s");
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_set_net", slot, 0, S)) return rc;
    if (desc) {
        if (int rc = check_net_desc(e->P.n_rays, e->P.eighth, *desc)) return rc;
        if (frame) if (int rc = check_net_frame(*desc, *frame)) return rc;
        if (rivals) if (int rc = check_net_rivals(*desc, frame, *rivals)) return rc;
        if (!params) return fail(FTGP_ERR_ARG, "ftgp_set_net: params is NULL%s");
    }
    HIP_TRY(hipSetDevice(e->device));
    if (!desc && !e->d_nets) return 0;        // nothing was ever defined
    if (int rc = ensure_nets(e)) return rc;
    NetDev N{};
    DevBuf<float> buf;
    if (desc) {
        N = net_record(*desc, frame, rivals);
        if (int rc = upload_params("ftgp_set_net", N, 1, (size_t)N.n_floats, params, buf)) return rc;
        N.params = buf.get();
    }
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the slot while it changes
    HIP_TRY(hipMemcpy(e->d_nets.get() + slot, &N, sizeof N, hipMemcpyHostToDevice));
    S->net = N;
    S->desc = desc ? *desc : FtgpNetDesc{};
    S->frame = (desc && frame && frame->enabled) ? *frame : FtgpNetFrame{};
    S->rivals = (desc && rivals && rivals->enabled) ? *rivals : FtgpNetRivals{};
    S->d_params = std::move(buf);                             // (the old buffer goes: nothing reads it any more)
    S->end_population();
    S->end_value();
    return 0;
}

int ftgp_set_net_device(FtgpEnv* e, void* stream, int slot, const float* params)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_set_net_device", slot, kSlotDefined | kSlotNoPopulation, S, "ftgp_set_net_population_device")) return rc;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = check_device_buffer(e, "ftgp_set_net_device", params, sizeof(float) * net_param_count(S->net), "params")) return rc;
    return on_handle_stream(e, stream, [&] { return launch_net_params(e, S->net, params, S->d_params.get(), 0, 1); });
}

int ftgp_get_net(FtgpEnv* e, int slot, FtgpNetDesc* desc_out, float* params_out)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_get_net", slot, kSlotDefined, S)) return rc;
    if (desc_out) *desc_out = S->desc;
    if (!params_out) return 0;
    HIP_TRY(hipSetDevice(e->device));
    return download_params(e, "ftgp_get_net", S->net, S->d_params.get(), params_out);
}

// ---- network populations: one parameter set per env (include/ftgp.h "Network populations") ----
int ftgp_set_net_population(FtgpEnv* e, int slot, int n_members, const float* params, const int32_t* env_member)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_set_net_population", slot, kSlotDefined, S)) return rc;
    const int n_envs = e->P.n_envs;
    if (n_members < 0 || n_members > n_envs) return failf(FTGP_ERR_ARG, "ftgp_set_net_population: n_members = %d outside 0 .. n_envs = %d", n_members, n_envs);
    if (n_members > 0 && !params) return fail(FTGP_ERR_ARG, "ftgp_set_net_population: params is NULL%s");
    if (n_members > 0 && env_member)
        for (int i = 0; i < n_envs; ++i)
            if (env_member[i] < 0 || env_member[i] >= n_members)
                return failf(FTGP_ERR_ARG, "ftgp_set_net_population: env_member[%d] = %d outside [0, n_members = %d)", i, env_member[i], n_members);
    HIP_TRY(hipSetDevice(e->device));
    NetDev N = S->net;
    DevBuf<float> buf;
    DevBuf<int32_t> map;
    if (n_members > 0) {
        std::vector<int32_t> members;
        if (int rc = net_host_buffer(members, (size_t)n_envs, "ftgp_set_net_population")) return rc;
        for (int i = 0; i < n_envs; ++i) members[(size_t)i] = env_member ? env_member[i] : i % n_members;
        if (int rc = upload_params("ftgp_set_net_population", N, n_members, (size_t)n_members * (size_t)net_member_stride(N.n_floats), params, buf)) return rc;
        HIP_TRY(dev_upload(map, members.data(), sizeof(int32_t) * members.size()));
        N.params = buf.get(); N.env_member = map.get();
    } else {
        if (!S->pop_members) return 0;                        // there is none
        N.params = S->d_params.get(); N.env_member = nullptr; // the slot's single set is in force again
    }
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the slot while it changes
    HIP_TRY(hipMemcpy(e->d_nets.get() + slot, &N, sizeof N, hipMemcpyHostToDevice));
    S->net = N;
    if (n_members > 0) {
        S->end_trainer();
        S->pop_members = n_members;
        S->d_pop_params = std::move(buf);                     // (the old buffers go: nothing reads them any more)
        S->d_pop_map = std::move(map);
    } else S->end_population();
    return 0;
}

int ftgp_set_net_population_device(FtgpEnv* e, void* stream, int slot, const float* params, const int32_t* env_member)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_set_net_population_device", slot, kSlotDefined | kSlotPopulation, S)) return rc;
    const int M = S->pop_members, n_envs = e->P.n_envs;
    HIP_TRY(hipSetDevice(e->device));
    const NetDev& N = S->net;
    if (params) if (int rc = check_device_buffer(e, "ftgp_set_net_population_device", params, sizeof(float) * net_param_count(N) * (size_t)M, "params")) return rc;
    if (env_member) if (int rc = check_device_buffer(e, "ftgp_set_net_population_device", env_member, sizeof(int32_t) * (size_t)n_envs, "env_member")) return rc;
    if (!params && !env_member) return 0;
    return on_handle_stream(e, stream, [&] {
        if (params) if (int rc = launch_net_params(e, N, params, S->d_pop_params.get(), net_member_stride(N.n_floats), M)) return rc;
        if (env_member) {
            hipLaunchKernelGGL(ftgp_net_map_kernel, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, e->stream.get(), env_member, S->d_pop_map.get(), n_envs, M);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    });
}

int ftgp_get_net_population(FtgpEnv* e, int slot, int32_t* n_members_out, int32_t* env_member_out, int member, float* params_out)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_get_net_population", slot, kSlotDefined, S)) return rc;
    const int M = S->pop_members;
    if (n_members_out) *n_members_out = M;
    if (!env_member_out && !params_out) return 0;
    if (int rc = net_slot(e, "ftgp_get_net_population", slot, kSlotPopulation, S)) return rc;
    if (params_out && (member < 0 || member >= M)) return failf(FTGP_ERR_ARG, "ftgp_get_net_population: member = %d outside [0, n_members = %d)", member, M);
    HIP_TRY(hipSetDevice(e->device));
    if (params_out)
        if (int rc = download_params(e, "ftgp_get_net_population", S->net, S->d_pop_params.get() + (size_t)member * (size_t)net_member_stride(S->net.n_floats), params_out)) return rc;
    if (env_member_out) {
        HIP_TRY(hipMemcpyAsync(env_member_out, S->d_pop_map.get(), sizeof(int32_t) * (size_t)e->P.n_envs, hipMemcpyDeviceToHost, e->stream.get()));
        HIP_TRY(hipStreamSynchronize(e->stream.get()));
    }
    return 0;
}

int ftgp_get_net_frame(FtgpEnv* e, int slot, FtgpNetFrame* frame_out)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_get_net_frame", slot, kSlotDefined, S)) return rc;
    if (frame_out) *frame_out = S->frame;
    return 0;
}

int ftgp_get_net_rivals(FtgpEnv* e, int slot, FtgpNetRivals* rivals_out)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_get_net_rivals", slot, kSlotDefined, S)) return rc;
    if (rivals_out) *rivals_out = S->rivals;
    return 0;
}

// ---- value nets: one critic per network slot (include/ftgp.h "Collected rollouts with values") ----
// what ftgp_set_value_net checks of a description; the message names the field
static int check_value_desc(const FtgpValueDesc& d)
{
    if (d.reserved != 0) return fail(FTGP_ERR_ARG, "ftgp_set_value_net: reserved must be 0%s");
    if (int rc = check_layers("ftgp_set_value_net", 1, d.n_layers, d.width, d.hidden_act, d.out_act)) return rc;
    if (!std::isfinite(d.out_scale)) return fail(FTGP_ERR_ARG, "ftgp_set_value_net: out_scale is not finite%s");
    if (!std::isfinite(d.out_offset)) return fail(FTGP_ERR_ARG, "ftgp_set_value_net: out_offset is not finite%s");
    return 0;
}

// the record of a value net on a slot of n_in inputs: NetDev's layer fields as net_layers reads them, the output map in entry 0, no
// scan, frame or rival fields (the inputs are the slot's) and no population
static NetDev value_record(const FtgpValueDesc& d, int n_in)
{
    NetDev N{};
    N.defined = 1; N.hidden_act = d.hidden_act; N.out_act = d.out_act;
    lay_out_layers(N, n_in, d.n_layers, d.width);
    N.out_scale[0] = d.out_scale; N.out_offset[0] = d.out_offset;
    return N;
}

int ftgp_set_value_net(FtgpEnv* e, int slot, const FtgpValueDesc* desc, const float* params)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_set_value_net", slot, kSlotDefined, S)) return rc;
    if (desc) {
        if (int rc = check_value_desc(*desc)) return rc;
        if (!params) return fail(FTGP_ERR_ARG, "ftgp_set_value_net: params is NULL%s");
    }
    if (!desc && !S->vnet.defined) return 0;                  // there is none
    HIP_TRY(hipSetDevice(e->device));
    NetDev N{};
    DevBuf<float> buf;
    DevBuf<NetDev> table;
    if (desc) {
        N = value_record(*desc, S->net.width[0]);
        if (int rc = upload_params("ftgp_set_value_net", N, 1, (size_t)N.n_floats, params, buf)) return rc;
        N.params = buf.get();
        if (!e->d_vnets) {                                    // the first value net of the handle: the records, every slot empty
            HIP_TRY(dev_alloc(table, sizeof(NetDev) * FTGP_MAX_NETS));
            HIP_TRY(hipMemset(table.get(), 0, sizeof(NetDev) * FTGP_MAX_NETS));
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is reading the record while it changes
    NetDev* records = table ? table.get() : e->d_vnets.get();
    HIP_TRY(hipMemcpy(records + slot, &N, sizeof N, hipMemcpyHostToDevice));
    if (table) e->d_vnets = std::move(table);
    S->end_value();                                           // (the old buffer goes: nothing reads it any more)
    if (desc) { S->vnet = N; S->vdesc = *desc; S->d_vparams = std::move(buf); }
    return 0;
}

int ftgp_set_value_net_device(FtgpEnv* e, void* stream, int slot, const float* params)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_set_value_net_device", slot, kSlotValue, S)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = check_device_buffer(e, "ftgp_set_value_net_device", params, sizeof(float) * net_param_count(S->vnet), "params")) return rc;
    return on_handle_stream(e, stream, [&] { return launch_net_params(e, S->vnet, params, S->d_vparams.get(), 0, 1); });
}

int ftgp_get_value_net(FtgpEnv* e, int slot, FtgpValueDesc* desc_out, float* params_out)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_get_value_net", slot, kSlotValue, S)) return rc;
    if (desc_out) *desc_out = S->vdesc;
    if (!params_out) return 0;
    HIP_TRY(hipSetDevice(e->device));
    return download_params(e, "ftgp_get_value_net", S->vnet, S->d_vparams.get(), params_out);
}

// ---- training on the device (include/ftgp.h "Training on the device") ----
static bool train_fraction(float b) { return std::isfinite(b) && b >= 0.0f && b < 1.0f; }

int ftgp_train_begin(FtgpEnv* e, int slot, const FtgpTrainDesc* desc)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_train_begin", slot, 0, S)) return rc;
    if (!desc) return fail(FTGP_ERR_ARG, "ftgp_train_begin: desc is NULL%s");
    if (!train_fraction(desc->beta1)) return fail(FTGP_ERR_ARG, "ftgp_train_begin: beta1 is not finite or outside [0, 1)%s");
    if (!train_fraction(desc->beta2)) return fail(FTGP_ERR_ARG, "ftgp_train_begin: beta2 is not finite or outside [0, 1)%s");
    if (!std::isfinite(desc->eps) || !(desc->eps > 0.0f)) return fail(FTGP_ERR_ARG, "ftgp_train_begin: eps is not finite or <= 0%s");
    if (desc->reserved != 0) return fail(FTGP_ERR_ARG, "ftgp_train_begin: reserved must be 0%s");
    if (int rc = net_slot(e, "ftgp_train_begin", slot, kSlotDefined | kSlotValue | kSlotNoPopulation | kSlotNoTrainer, S)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    FtgpEnv::Trainer T;
    T.desc = *desc;
    T.n[0] = S->net.n_floats; T.n[1] = S->vnet.n_floats;
    const size_t total = (size_t)T.n[0] + (size_t)T.n[1];
    HIP_TRY(dev_zeros(T.grad, sizeof(float) * total, e->stream.get()));
    HIP_TRY(dev_zeros(T.m, sizeof(float) * total, e->stream.get()));
    HIP_TRY(dev_zeros(T.v, sizeof(float) * total, e->stream.get()));
    HIP_TRY(dev_zeros(T.part, sizeof(float) * total * FTGP_TRAIN_MAX_WG, e->stream.get()));
    // (the workgroups' stats, the trainer's own, then the workgroups' binary64 sums: four doubles each)
    HIP_TRY(dev_zeros(T.stats, sizeof(float) * FTGP_TRAIN_STATS * (2 * FTGP_TRAIN_MAX_WG + 1), e->stream.get()));
    HIP_TRY(dev_zeros(T.sync, sizeof(int32_t) * 2, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    T.on = true;
    S->trainer = std::move(T);
    return 0;
}

int ftgp_train_end(FtgpEnv* e, int slot)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_train_end", slot, kSlotTrainer, S)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));           // no launch is using the buffers while they go
    S->end_trainer();
    return 0;
}

// one of a slot's nets as the train kernels read it; x_off: where the layers' outputs sit in an LDS row (the input at 0)
static TrainNet train_net(const NetDev& N, const float* params, int g_off)
{
    TrainNet t{};
    t.n_layers = N.n_layers; t.hidden_act = N.hidden_act; t.out_act = N.out_act; t.n_floats = N.n_floats;
    int x = 0;
    for (int l = 0; l <= N.n_layers; ++l) {
        t.width[l] = N.width[l]; t.x_off[l] = x; x += (N.width[l] + 3) & ~3;
        if (l < N.n_layers) { t.w_off[l] = N.w_off[l]; t.b_off[l] = N.b_off[l]; }
    }
    for (int k = 0; k < 2; ++k) { t.out_scale[k] = N.out_scale[k]; t.out_offset[k] = N.out_offset[k]; }
    t.params = params; t.g_off = g_off;
    return t;
}

int ftgp_train_grad_device(FtgpEnv* e, const FtgpTrainBatch* b)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (!b) return fail(FTGP_ERR_ARG, "ftgp_train_grad_device: the batch is NULL%s");
    static const char* const entry = "ftgp_train_grad_device";
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, entry, b->slot, kSlotTrainer, S)) return rc;
    FtgpEnv::Trainer& R = S->trainer;
    if (b->reserved[0] != 0 || b->reserved[1] != 0) return fail(FTGP_ERR_ARG, "ftgp_train_grad_device: reserved must be 0%s");
    if (b->n_rows < 1) return failf(FTGP_ERR_ARG, "ftgp_train_grad_device: n_rows = %d must be >= 1", b->n_rows);
    if (b->n_batch < 1) return failf(FTGP_ERR_ARG, "ftgp_train_grad_device: n_batch = %d must be >= 1", b->n_batch);
    if (!b->index && (b->first_row < 0 || (int64_t)b->first_row + (int64_t)b->n_batch > (int64_t)b->n_rows))
        return failf(FTGP_ERR_ARG, "ftgp_train_grad_device: first_row = %d with n_batch = %d leaves the %d rows", b->first_row, b->n_batch, b->n_rows);
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(b->std[k]) || !(b->std[k] > 0.0f)) return failf(FTGP_ERR_ARG, "ftgp_train_grad_device: std[%d] is not finite or <= 0", k);
    if (!std::isfinite(b->clip) || b->clip < 0.0f) return fail(FTGP_ERR_ARG, "ftgp_train_grad_device: clip is not finite or < 0%s");
    if (!std::isfinite(b->value_coef) || b->value_coef < 0.0f) return fail(FTGP_ERR_ARG, "ftgp_train_grad_device: value_coef is not finite or < 0%s");
    HIP_TRY(hipSetDevice(e->device));
    const NetDev& N = S->net; const NetDev& V = S->vnet;
    const size_t rows = (size_t)b->n_rows, B = (size_t)b->n_batch, n_in = (size_t)N.width[0];
    if (b->index) if (int rc = check_device_buffer(e, entry, b->index, sizeof(int32_t) * B, "index")) return rc;
    if (int rc = check_device_buffer(e, entry, b->inputs, sizeof(float) * rows * n_in, "inputs")) return rc;
    if (int rc = check_device_buffer(e, entry, b->mean, sizeof(float) * rows * 2, "mean")) return rc;
    if (b->noise) if (int rc = check_device_buffer(e, entry, b->noise, sizeof(float) * rows * 2, "noise")) return rc;
    if (int rc = check_device_buffer(e, entry, b->advantage, sizeof(float) * rows, "advantage")) return rc;
    if (int rc = check_device_buffer(e, entry, b->ret, sizeof(float) * rows, "ret")) return rc;
    if (b->weight) if (int rc = check_device_buffer(e, entry, b->weight, sizeof(float) * rows, "weight")) return rc;
    if (b->stats) if (int rc = check_device_buffer(e, entry, b->stats, sizeof(float) * FTGP_TRAIN_STATS, "stats")) return rc;
    if (b->new_mean) if (int rc = check_device_buffer(e, entry, b->new_mean, sizeof(float) * B * 2, "new_mean")) return rc;
    if (b->new_value) if (int rc = check_device_buffer(e, entry, b->new_value, sizeof(float) * B, "new_value")) return rc;

    TrainArgs T{};
    T.net[0] = train_net(N, S->d_params.get(), 0);
    T.net[1] = train_net(V, S->d_vparams.get(), R.n[0]);
    int act_floats = 0, ld_max = FTGP_WAVE;
    for (int w = 0; w < 2; ++w) {
        const TrainNet& t = T.net[w];
        act_floats = std::max(act_floats, t.x_off[t.n_layers] + ((t.width[t.n_layers] + 3) & ~3));
        for (int l = 1; l <= t.n_layers; ++l) ld_max = std::max(ld_max, (t.width[l] + FTGP_WAVE - 1) & ~(FTGP_WAVE - 1));
    }
    T.d_off[0] = act_floats; T.d_off[1] = act_floats + ld_max;
    T.row_floats = act_floats + 2 * ld_max;                   // a multiple of 4 ...
    if ((T.row_floats / 4) % 2 == 0) T.row_floats += 4;       // ... and an odd one: rows a thread apart fall into different banks
    const int tile = (size_t)32 * (size_t)T.row_floats * sizeof(float) <= 63 * 1024 ? 32 : 16;
    T.n_rows = b->n_rows; T.n_batch = b->n_batch; T.first_row = b->first_row;
    T.n_tiles = (int)((B + (size_t)tile - 1) / (size_t)tile);
    T.n_total = R.n[0] + R.n[1];
    T.index = b->index; T.inputs = b->inputs; T.mean = b->mean; T.noise = b->noise; T.advantage = b->advantage; T.ret = b->ret; T.weight = b->weight;
    T.std[0] = b->std[0]; T.std[1] = b->std[1]; T.clip = b->clip; T.value_coef = b->value_coef;
    T.new_mean = b->new_mean; T.new_value = b->new_value;
    T.part = R.part.get(); T.part_stats = R.stats.get();
    static_assert(((FTGP_TRAIN_MAX_WG + 1) * FTGP_TRAIN_STATS * sizeof(float)) % alignof(double) == 0 && 4 * sizeof(double) <= FTGP_TRAIN_STATS * sizeof(float), "the binary64 sums behind the stats");
    T.part_wide = reinterpret_cast<double*>(R.stats.get() + (size_t)(FTGP_TRAIN_MAX_WG + 1) * FTGP_TRAIN_STATS);      // [FTGP_TRAIN_MAX_WG][4]
    const int G = std::min(T.n_tiles, FTGP_TRAIN_MAX_WG);
    const size_t lds = (size_t)tile * (size_t)T.row_floats * sizeof(float);

    return on_handle_stream(e, b->stream, [&] {
        if (tile == 32) hipLaunchKernelGGL(ftgp_train_grad_kernel<32>, dim3((unsigned)G), dim3(FTGP_TRAIN_THREADS), lds, e->stream.get(), T);
        else hipLaunchKernelGGL(ftgp_train_grad_kernel<16>, dim3((unsigned)G), dim3(FTGP_TRAIN_THREADS), lds, e->stream.get(), T);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(R.sync.get(), 0, sizeof(int32_t) * 2, e->stream.get()));
        TrainReduceArgs A{};
        A.part = R.part.get(); A.part_stats = R.stats.get(); A.part_wide = T.part_wide; A.G = G; A.n_total = T.n_total;
        A.grad = R.grad.get(); A.sync = R.sync.get(); A.stats = R.stats.get() + (size_t)FTGP_TRAIN_MAX_WG * FTGP_TRAIN_STATS; A.stats_out = b->stats;
        hipLaunchKernelGGL(ftgp_train_reduce_kernel, dim3((unsigned)((T.n_total + 255) / 256)), dim3(256), 0, e->stream.get(), A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int ftgp_train_adam_device(FtgpEnv* e, void* stream, int slot, float lr)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_train_adam_device", slot, 0, S)) return rc;
    if (!std::isfinite(lr) || lr < 0.0f) return fail(FTGP_ERR_ARG, "ftgp_train_adam_device: lr is not finite or < 0%s");
    if (int rc = net_slot(e, "ftgp_train_adam_device", slot, kSlotTrainer, S)) return rc;
    FtgpEnv::Trainer& R = S->trainer;
    HIP_TRY(hipSetDevice(e->device));
    return on_handle_stream(e, stream, [&] {
        R.t += 1;
        float s[6];
        ftgp_adam_scalars(R.desc.beta1, R.desc.beta2, lr, R.t, s);
        TrainAdamArgs A{};
        A.p[0] = S->d_params.get(); A.p[1] = S->d_vparams.get(); A.n[0] = R.n[0]; A.n[1] = R.n[1];
        A.grad = R.grad.get(); A.m = R.m.get(); A.v = R.v.get(); A.sync = R.sync.get();
        A.b1 = s[0]; A.b2 = s[1]; A.omb1 = s[2]; A.omb2 = s[3]; A.a = s[4]; A.r = s[5]; A.eps = R.desc.eps;
        hipLaunchKernelGGL(ftgp_train_adam_kernel, dim3((unsigned)((R.n[0] + R.n[1] + 255) / 256)), dim3(256), 0, e->stream.get(), A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int ftgp_train_get(FtgpEnv* e, int slot, int what, float* policy_out, float* value_out, int64_t* steps_out)
{
    FtgpEnv::NetSlot* S;
    if (int rc = net_slot(e, "ftgp_train_get", slot, 0, S)) return rc;
    if (what < FTGP_TRAIN_GRAD || what > FTGP_TRAIN_RAW_PARAMS) return failf(FTGP_ERR_ARG, "ftgp_train_get: what = %d is no FTGP_TRAIN_*", what);
    if (int rc = net_slot(e, "ftgp_train_get", slot, kSlotTrainer, S)) return rc;
    FtgpEnv::Trainer& R = S->trainer;
    if (steps_out) *steps_out = R.t;
    if (!policy_out && !value_out) return 0;
    HIP_TRY(hipSetDevice(e->device));
    if (what >= FTGP_TRAIN_RAW_GRAD) {                         // the library's layout as it lies in device memory, padding included
        const bool g = what == FTGP_TRAIN_RAW_GRAD;
        if (policy_out) HIP_TRY(hipMemcpyAsync(policy_out, g ? R.grad.get() : S->d_params.get(), sizeof(float) * (size_t)R.n[0], hipMemcpyDeviceToHost, e->stream.get()));
        if (value_out) HIP_TRY(hipMemcpyAsync(value_out, g ? R.grad.get() + R.n[0] : S->d_vparams.get(), sizeof(float) * (size_t)R.n[1], hipMemcpyDeviceToHost, e->stream.get()));
        HIP_TRY(hipStreamSynchronize(e->stream.get()));
        return 0;
    }
    const float* src = what == FTGP_TRAIN_GRAD ? R.grad.get() : what == FTGP_TRAIN_M ? R.m.get() : R.v.get();
    if (policy_out) if (int rc = download_params(e, "ftgp_train_get", S->net, src, policy_out)) return rc;
    if (value_out) if (int rc = download_params(e, "ftgp_train_get", S->vnet, src + R.n[0], value_out)) return rc;
    return 0;
}

int ftgp_env_state_bytes(FtgpEnv* e, size_t* bytes_per_env)
{
    if (!e || !bytes_per_env) return fail(FTGP_ERR_ARG, "null argument%s");
    *bytes_per_env = env_state_bytes(e->P);
    return 0;
}

// the checks ftgp_save_envs_device and ftgp_load_envs_device (`entry`) share; `need_all`: row e of every env must exist
static int env_state_checks(FtgpEnv* e, const char* entry, const void* rows, int64_t n_rows, bool need_all, const void* per_env, size_t per_env_bytes, const char* per_env_name)
{
    if (n_rows < 1 || n_rows > 0x7fffffffll) return failf(FTGP_ERR_ARG, "%s: n_rows = %lld, not in 1 .. 2^31 - 1", entry, (long long)n_rows);
    if (need_all && n_rows < e->P.n_envs) return failf(FTGP_ERR_ARG, "%s: n_rows = %lld, fewer than the handle's %d envs", entry, (long long)n_rows, e->P.n_envs);
    if (int rc = check_device_buffer(e, entry, rows, env_state_bytes(e->P) * (size_t)n_rows, "rows")) return rc;
    if ((uintptr_t)rows % 16 != 0) return failf(FTGP_ERR_ARG, "%s: rows is not 16-byte aligned", entry);
    if (per_env) if (int rc = check_device_buffer(e, entry, per_env, per_env_bytes, per_env_name)) return rc;
    return 0;
}

int ftgp_save_envs_device(FtgpEnv* e, void* stream, void* rows, int64_t n_rows, const uint8_t* env_mask)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = env_state_checks(e, "ftgp_save_envs_device", rows, n_rows, true, env_mask, (size_t)e->P.n_envs, "env_mask")) return rc;
    if (int rc = ensure_env_state(e)) return rc;
    EnvStateArgs A = env_state_args(e, rows, n_rows);
    A.env_mask = env_mask;
    return on_handle_stream(e, stream, [&] {
        hipLaunchKernelGGL(ftgp_env_save_kernel, dim3(env_state_blocks(e)), dim3(FTGP_ENV_STATE_THREADS), 0, e->stream.get(), e->P, A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int ftgp_load_envs_device(FtgpEnv* e, void* stream, const void* rows, int64_t n_rows, const int32_t* src_row)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = env_state_checks(e, "ftgp_load_envs_device", rows, n_rows, !src_row, src_row, sizeof(int32_t) * (size_t)e->P.n_envs, "src_row")) return rc;
    if (int rc = ensure_env_state(e)) return rc;
    EnvStateArgs A = env_state_args(e, const_cast<void*>(rows), n_rows);
    A.src_row = src_row;
    return on_handle_stream(e, stream, [&] {
        hipLaunchKernelGGL(ftgp_env_load_kernel, dim3(env_state_blocks(e)), dim3(FTGP_ENV_STATE_THREADS), 0, e->stream.get(), e->P, A);
        HIP_TRY(hipGetLastError());
        e->rows_valid = false; e->launch_metrics_valid = false;
        return 0;
    });
}

int ftgp_get_env_state_rejected(FtgpEnv* e, int64_t* rejected)
{
    if (!e || !rejected) return fail(FTGP_ERR_ARG, "null argument%s");
    *rejected = 0;
    if (!e->d_state_aux) return 0;          // no load yet
    HIP_TRY(hipSetDevice(e->device));
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, &e->d_state_aux.get()->rejected, sizeof n, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    *rejected = (int64_t)n;
    return 0;
}

int ftgp_obs_device(FtgpEnv* e, void* stream, float* obs)
{
    const size_t n_beams = e && e->ds.ready ? (size_t)e->ds.sig.n_beams : 1;
    return rows_to_device(e, "ftgp_obs_device", stream, n_beams, obs, "obs", [&] {
        DeviceIoArgs A = e->ds.io;
        DeviceSignalArgs S = e->ds.sig;
        A.obs = obs;
        const bool aligned = (uintptr_t)obs % 16 == 0;          // as a device step chooses (ftgp_step_device_rivals)
        S.vec_out = aligned && S.n_beams % 4 == 0;
        if (S.path == FTGP_SIG_PATH_REGS && !aligned) S.path = FTGP_SIG_PATH_STAGE;
        hipLaunchKernelGGL(ftgp_io_obs_kernel, dim3((unsigned)e->P.n_envs), dim3(FTGP_IO_THREADS), 0, e->stream.get(), e->P, A, S);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int ftgp_get_episodes(FtgpEnv* e, int64_t* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    const size_t bytes = sizeof(int64_t) * (size_t)e->P.n_envs;
    if (!e->d_episodes) { memset(out, 0, bytes); return 0; }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(out, e->d_episodes.get(), bytes, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_start_table(FtgpEnv* e, int track, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (track < 0 || track >= e->n_tracks) return failf(FTGP_ERR_ARG, "ftgp_get_start_table: track %d of a handle with %d", track, e->n_tracks);
    memcpy(out, &e->start_table[6 * FTGP_PATH_POINTS * (size_t)track], sizeof(double) * 6 * FTGP_PATH_POINTS);
    return 0;
}

int ftgp_get_contacts(FtgpEnv* e, float* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_contact_rows(e)) return rc;
    if (int rc = launch_contacts(e, e->ds.d_contact.get(), nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->ds.d_contact.get(), sizeof(float) * FTGP_CONTACT_FLOATS * (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_frames(FtgpEnv* e, int n_ahead, int stride, float* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (n_ahead < 0 || n_ahead > FTGP_MAX_LOOKAHEAD) return fail(FTGP_ERR_ARG, "ftgp_get_frames: n_ahead in 0 .. 16%s");
    if (stride < 1 || stride > FTGP_PATH_POINTS / 2) return fail(FTGP_ERR_ARG, "ftgp_get_frames: stride in 1 .. 50%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_frame_rows(e)) return rc;
    if (int rc = launch_frame(e, n_ahead, stride, e->ds.d_frame.get(), nullptr, -1)) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->ds.d_frame.get(), sizeof(float) * (size_t)(FTGP_FRAME_FIXED + 2 * n_ahead) * (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_rivals(FtgpEnv* e, int n_rivals, float* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (n_rivals < 0 || n_rivals > FTGP_MAX_RIVALS) return fail(FTGP_ERR_ARG, "ftgp_get_rivals: n_rivals in 0 .. 7%s");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_rival_rows(e)) return rc;
    if (int rc = launch_rivals_now(e, n_rivals, e->ds.d_rival.get(), nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->ds.d_rival.get(), sizeof(float) * (size_t)(FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * n_rivals) * (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_lidar(FtgpEnv* e, float* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy2DAsync(out, sizeof(float) * (size_t)e->P.n_rays, e->d_ranges.get(), sizeof(float) * (size_t)e->P.ranges_stride,
                             sizeof(float) * (size_t)e->P.n_rays, (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_snapshot(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    for (int i = 0; i < e->P.n_cars; ++i) {
        const double* a = e->h_core.data() + (size_t)i * kCoreDoubles;
        double* o = out + (size_t)i * FTGP_SNAPSHOT_DOUBLES;
        // quaternion_to_euler(w, 0, 0, z), custom.py:62-76
        const double w = a[2], x = 0.0, y = 0.0, z = a[3];
        const double roll = atan2(+2.0 * (w * x + y * z), +1.0 - 2.0 * (x * x + y * y));
        double t2 = +2.0 * (w * y - z * x);
        t2 = t2 > +1.0 ? +1.0 : t2; t2 = t2 < -1.0 ? -1.0 : t2;
        const double pitch = asin(t2);
        const double yaw = atan2(+2.0 * (w * z + x * y), +1.0 - 2.0 * (y * y + z * z));
        o[0] = a[9]; o[1] = a[4]; o[2] = a[5]; o[3] = 0.0; o[4] = yaw; o[5] = pitch; o[6] = roll;
        o[7] = a[10]; o[8] = a[11];
        o[9] = a[12] / e->P.dt;   // time = steps / timestep, custom.py:1397 (sic)
    }
    return 0;
}

int ftgp_get_pose(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    for (int i = 0; i < e->P.n_cars; ++i) {
        const double* a = e->h_core.data() + (size_t)i * kCoreDoubles;
        double* o = out + (size_t)i * FTGP_POSE_DOUBLES;
        o[0] = a[0]; o[1] = a[1]; o[2] = e->P.veh.body_z; o[3] = a[2]; o[4] = 0; o[5] = 0; o[6] = a[3];
        o[7] = a[4]; o[8] = a[5]; o[9] = 0; o[10] = 0; o[11] = 0; o[12] = a[6];
    }
    return 0;
}

int ftgp_set_pose(FtgpEnv* e, const double* pose)
{
    if (!e || !pose) return fail(FTGP_ERR_ARG, "null argument%s");
    e->rows_valid = false; e->launch_metrics_valid = false;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(e->d_pose.get(), pose, sizeof(double) * FTGP_POSE_DOUBLES * (size_t)e->P.n_cars, hipMemcpyHostToDevice, e->stream.get()));
    hipLaunchKernelGGL(ftgp_set_pose_kernel, dim3((e->P.n_cars + 255) / 256), dim3(256), 0, e->stream.get(), e->P, e->d_pose.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_policy_eval(FtgpEnv* e, int policy, const float* ranges, double* ctrl_out)
{
    if (!e || !ranges) return fail(FTGP_ERR_ARG, "null argument%s");
    e->rows_valid = false;
    if (policy < FTGP_POLICY_LOBOTOMY || policy > FTGP_POLICY_NET3) return fail(FTGP_ERR_ARG, "policy_eval: device policies only%s");
    if (policy == FTGP_POLICY_PER_CAR && !e->P.car_policy[0]) return fail(FTGP_ERR_STATE, "FTGP_POLICY_PER_CAR without ftgp_set_car_policies%s");
    if (int rc = check_nets_defined(e, nets_named(e, policy, false))) return rc;
    if (uses_disparity_driver(e, policy)) if (int rc = check_disparity_shape(e->P)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy2DAsync(e->d_ranges.get(), sizeof(float) * (size_t)e->P.ranges_stride, ranges, sizeof(float) * (size_t)e->P.n_rays,
                             sizeof(float) * (size_t)e->P.n_rays, (size_t)e->P.n_cars, hipMemcpyHostToDevice, e->stream.get()));
    const size_t lds = 4 * ((size_t)e->P.win_floats * sizeof(float) + sizeof(CarCore) + FTGP_WAVE * sizeof(int));
    if (lds > 64 * 1024) return fail(FTGP_ERR_ARG, "scan does not fit LDS%s");
    hipLaunchKernelGGL(ftgp_policy_kernel, dim3((e->P.n_cars + 3) / 4), dim3(256), lds, e->stream.get(), e->P, policy, ctrl_out ? e->d_ctrl.get() : nullptr,
                       (const int32_t*)e->d_env_track.get());
    HIP_TRY(hipGetLastError());
    if (ctrl_out) HIP_TRY(hipMemcpyAsync(ctrl_out, e->d_ctrl.get(), sizeof(double) * 2 * (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_eval_progress(FtgpEnv* e)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    e->rows_valid = false; e->launch_metrics_valid = false;
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(ftgp_progress_kernel, dim3((e->P.n_cars + 63) / 64), dim3(64), 0, e->stream.get(), e->P, (const int32_t*)e->d_env_track.get());
    HIP_TRY(hipGetLastError());
    return 0;
}

int ftgp_get_progress(FtgpEnv* e, int32_t* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    memcpy(out, e->h_prog.data(), sizeof(int32_t) * e->h_prog.size());
    return 0;
}

int ftgp_get_centre_dist2(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy2DAsync(out, sizeof(double), reinterpret_cast<const char*>(e->d_cars.get()) + offsetof(CarCore, dist2), sizeof(CarState),
                             sizeof(double), (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_winners(FtgpEnv* e, int32_t* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    // places in the order cars reached lap_target; cars that got there in the same step rank in car order, the order of the
    // reference's per-car loop (custom.py:1337,1367-1369)
    const int cpe = e->P.cars_per_env;
    for (int env = 0; env < e->P.n_envs; ++env) {
        const int32_t* p = e->h_prog.data() + (size_t)env * cpe * FTGP_PROGRESS_INTS;
        for (int i = 0; i < cpe; ++i) {
            int place = 0;
            if (p[i * FTGP_PROGRESS_INTS + 4]) {
                place = 1;
                auto fin64 = [&](int k) { int64_t v; memcpy(&v, e->h_core.data() + ((size_t)env * cpe + k) * kCoreDoubles + 15, sizeof v); return v; };      // all 64 bits
                const int64_t mine = fin64(i);
                for (int k = 0; k < cpe; ++k)
                    if (k != i && p[k * FTGP_PROGRESS_INTS + 4]) {
                        const int64_t theirs = fin64(k);
                        if (theirs < mine || (theirs == mine && k < i)) ++place;
                    }
            }
            out[(size_t)env * cpe + i] = place;
        }
    }
    return 0;
}

int ftgp_get_lap_times(FtgpEnv* e, int32_t* counts, double* times)
{
    if (!e || !counts || !times) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    for (int i = 0; i < e->P.n_cars; ++i) counts[i] = (int32_t)e->h_core[(size_t)i * kCoreDoubles + 13];
    HIP_TRY(hipMemcpy2DAsync(times, sizeof(double) * FTGP_MAX_LAP_TIMES, reinterpret_cast<const char*>(e->d_cars.get()) + sizeof(CarCore), sizeof(CarState),   // times[] follows the CarCore head
                            
                             sizeof(double) * FTGP_MAX_LAP_TIMES, (size_t)e->P.n_cars, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

int ftgp_get_race_steps(FtgpEnv* e, int64_t* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    for (int i = 0; i < e->P.n_cars; ++i) {          // the pack kernel ships the two int64 as bit patterns in the row's last two doubles
        memcpy(out + 2 * (size_t)i, e->h_core.data() + (size_t)i * kCoreDoubles + 14, sizeof(int64_t));
        memcpy(out + 2 * (size_t)i + 1, e->h_core.data() + (size_t)i * kCoreDoubles + 15, sizeof(int64_t));
    }
    return 0;
}

int ftgp_get_ctrl(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = sync_rows_to_host(e)) return rc;
    for (int i = 0; i < e->P.n_cars; ++i) { out[2 * i] = e->h_core[(size_t)i * kCoreDoubles + 7]; out[2 * i + 1] = e->h_core[(size_t)i * kCoreDoubles + 8]; }
    return 0;
}

int ftgp_get_steps(FtgpEnv* e, int64_t* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(out, e->d_steps.get(), sizeof(int64_t) * (size_t)e->P.n_envs, hipMemcpyDeviceToHost, e->stream.get()));
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    return 0;
}

// the record of this GPU: the step kernel's last workgroup has written it into pinned memory (slot cur_slot), or ftgp_metrics_kernel does now
static int metrics_to_host(FtgpEnv* e, double* out)
{
    if (!e->launch_metrics_valid) {
        // An exchange that was begun on this very slot and not ended yet (one rank: its "exchange" IS the slot in pinned memory) promised the
        // record of the state at its begin: put that aside before the slot is refreshed with the present state's.
        if (e->gather_open && e->gather_slot == e->cur_slot && !e->comm && !e->gather_held) {
            HIP_TRY(hipEventSynchronize(e->gather_event));
            collect_slot(e, e->cur_slot, e->held);
            e->gather_held = true;
        }
        hipLaunchKernelGGL(ftgp_metrics_kernel, dim3(1), dim3(FTGP_METRIC_THREADS), 0, e->stream.get(), e->P, e->h_metrics_dev + (size_t)e->cur_slot * FTGP_METRIC_DOUBLES);
        HIP_TRY(hipGetLastError());
        e->slot_partial[e->cur_slot] = false;
    }
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    collect_slot(e, e->cur_slot, out);
    return 0;
}

int ftgp_metrics_local(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    HIP_TRY(hipSetDevice(e->device));
    return metrics_to_host(e, out);
}

int ftgp_comm_unique_id(uint8_t id_out[128])
{
    if (!id_out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = load_rccl()) return rc;
    Id128 id;
    int r = g_rccl.GetUniqueId(&id);
    if (r != 0) return fail(FTGP_ERR_COMM, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    memcpy(id_out, id.internal, 128);
    return 0;
}

int ftgp_comm_init(FtgpEnv* e, const uint8_t id[128], int rank, int world_size)
{
    if (!e || !id || world_size < 1 || rank < 0 || rank >= world_size) return fail(FTGP_ERR_ARG, "bad comm arguments%s");
    if (e->comm) return fail(FTGP_ERR_STATE, "the handle already has a communicator%s");
    if (e->n_tracks > 1) return fail(FTGP_ERR_STATE, "ftgp_comm_init: multi-rank runs of a multi-track handle are not supported%s");
    if (int rc = load_rccl()) return rc;
    HIP_TRY(hipSetDevice(e->device));
    Id128 uid; memcpy(uid.internal, id, 128);
    // the gathered records get buffers of their own (this rank's record slots, h_metrics, written by the step kernel, stay untouched) -- allocated
    // BEFORE the communicator: a handle never holds a communicator without them
    DevBuf<double> d_gather; HostBuf<double> h_gather;
    if (dev_alloc(d_gather, sizeof(double) * FTGP_METRIC_DOUBLES * (size_t)world_size) != hipSuccess ||
        host_alloc(h_gather, sizeof(double) * FTGP_METRIC_DOUBLES * (size_t)world_size, hipHostMallocDefault) != hipSuccess)
        return fail(FTGP_ERR_HIP, "ftgp_comm_init: no memory for the gathered records%s");
    // launches from here on leave their record on the device (no partial records to the host); one still in flight finishes first (nothing is enqueued after it)
    HIP_TRY(hipStreamSynchronize(e->stream.get()));
    void* comm = nullptr;
    int r = g_rccl.CommInitRank(&comm, world_size, uid, rank);
    if (r != 0) return fail(FTGP_ERR_COMM, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    e->comm = comm; e->d_gather = std::move(d_gather); e->h_gather = std::move(h_gather);
    e->rank = rank; e->world = world_size;
    return 0;
}

int ftgp_metrics_allgather_begin(FtgpEnv* e)
{
    if (!e) return fail(FTGP_ERR_ARG, "null handle%s");
    if (e->gather_open) return fail(FTGP_ERR_STATE, "ftgp_metrics_allgather_begin: the previous exchange has not been ended%s");
    HIP_TRY(hipSetDevice(e->device));
    const int slot = e->cur_slot;
    const size_t so = (size_t)slot * FTGP_METRIC_DOUBLES;
    const bool rccl = e->comm != nullptr;            // a one-rank communicator goes through RCCL too (that is how one GPU tests the path)
    // a communicator that arrived after a launch whose record went to the host as partial records: the device has no copy of that record
    const bool refresh = !e->launch_metrics_valid || (rccl && e->slot_partial[slot]);
    if (refresh) {                       // otherwise the slot already holds this state's record (step kernel epilogue), on the device and in pinned memory
        hipLaunchKernelGGL(ftgp_metrics_kernel, dim3(1), dim3(FTGP_METRIC_THREADS), 0, e->stream.get(), e->P, rccl ? e->d_metrics.get() + so : e->h_metrics_dev + so);
        HIP_TRY(hipGetLastError());
        e->slot_partial[slot] = false;
    }
    e->gather_held = false;
    if (!rccl) {                         // one rank: the "exchange" is the record's arrival in pinned memory
        if (!refresh && e->timed) e->gather_event = e->ev_stop[slot].get();      // ... with the launch that wrote it: nothing to enqueue
        else { HIP_TRY(hipEventRecord(e->ev_gather.get(), e->stream.get())); e->gather_event = e->ev_gather.get(); }
    } else {
        // the record is produced on the compute stream; everything else happens on the side stream, beside the next launch
        // (the launch's own stop event -- it rides on the kernel's dispatch packet -- says when the record is there.  An event of its own, recorded behind the
        // launch, is a barrier packet with a system-scope fence between this launch and the next: measured with a one-rank communicator, the next launch then runs
        // 20 - 25 us longer -- it finds the L2s flushed -- whatever the exchange itself does: profiles/round5/exchange_overlap_one_rank.log)
        hipEvent_t ready = (!refresh && e->timed) ? e->ev_stop[slot].get() : e->ev_metrics.get();
        if (ready == e->ev_metrics.get()) HIP_TRY(hipEventRecord(e->ev_metrics.get(), e->stream.get()));
        HIP_TRY(hipStreamWaitEvent(e->side.get(), ready, 0));
        int r = g_rccl.AllGather(e->d_metrics.get() + so, e->d_gather.get(), FTGP_METRIC_DOUBLES, kNcclFloat64, e->comm, e->side.get());
        if (r != 0) return fail(FTGP_ERR_COMM, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
        HIP_TRY(hipMemcpyAsync(e->h_gather.get(), e->d_gather.get(), sizeof(double) * FTGP_METRIC_DOUBLES * (size_t)e->world, hipMemcpyDeviceToHost, e->side.get()));
        HIP_TRY(hipEventRecord(e->ev_gather.get(), e->side.get()));
        e->gather_event = e->ev_gather.get();
    }
    e->gather_open = true; e->gather_slot = slot;
    return 0;
}

int ftgp_metrics_allgather_end(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (!e->gather_open) return fail(FTGP_ERR_STATE, "ftgp_metrics_allgather_end without _begin%s");
    HIP_TRY(hipSetDevice(e->device));
    if (!e->gather_held) HIP_TRY(hipEventSynchronize(e->gather_event));      // this exchange only: a later launch on the compute stream is not waited for
    e->gather_open = false;
    if (e->comm) memcpy(out, e->h_gather.get(), sizeof(double) * FTGP_METRIC_DOUBLES * (size_t)e->world);
    else if (e->gather_held) memcpy(out, e->held, sizeof e->held);
    else collect_slot(e, e->gather_slot, out);
    return 0;
}

int ftgp_metrics_allgather(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = ftgp_metrics_allgather_begin(e)) return rc;
    return ftgp_metrics_allgather_end(e, out);
}

int ftgp_get_track_distance_field(FtgpEnv* e, int track, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (track < 0 || track >= e->n_tracks) return failf(FTGP_ERR_ARG, "get_track_distance_field: track %d of a handle with %d", track, e->n_tracks);
    const TrackBufs& b = e->trk[(size_t)track];
    if (!b.edt) return fail(FTGP_ERR_STATE, "no distance field: the handle was not created with lidar_mode = FTGP_LIDAR_FAKELIDAR%s");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(out, b.edt.get(), sizeof(double) * (size_t)b.width * b.height, hipMemcpyDeviceToHost));
    return 0;
}

int ftgp_get_distance_field(FtgpEnv* e, double* out)
{
    if (!e || !out) return fail(FTGP_ERR_ARG, "null argument%s");
    if (e->n_tracks > 1) return fail(FTGP_ERR_STATE, "get_distance_field: the handle has several tracks (ftgp_get_track_distance_field)%s");
    return ftgp_get_track_distance_field(e, 0, out);
}

int ftgp_fakelidar(int device_id, const double* dt, int H, int W, int n_origins, const double* origins, int rangefinders,
                   const double* cosines, const double* sines, double eps, double* scan, double* points)
{
    if (!dt || !origins || !cosines || !sines || !scan || !points || H < 1 || W < 1 || n_origins < 1 || rangefinders < 1)
        return fail(FTGP_ERR_ARG, "fakelidar: bad argument%s");
    if (int rc = open_device(device_id)) return rc;
    const size_t n = (size_t)n_origins * rangefinders, ndt = (size_t)H * W;
    DevBuf<double> d_dt, d_o, d_c, d_s, d_scan, d_pts; DevBuf<int> d_err; int herr = 0;
    HIP_TRY(dev_upload(d_dt, dt, ndt * 8)); HIP_TRY(dev_upload(d_o, origins, (size_t)n_origins * 16)); HIP_TRY(dev_upload(d_c, cosines, n * 8)); HIP_TRY(dev_upload(d_s, sines, n * 8));
    HIP_TRY(dev_alloc(d_scan, n * 8)); HIP_TRY(dev_alloc(d_pts, n * 16)); HIP_TRY(dev_alloc(d_err, 4));
    HIP_TRY(hipMemset(d_err.get(), 0, 4));
    hipLaunchKernelGGL(ftgp_fakelidar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_dt.get(), H, W, (int)n, rangefinders, d_o.get(), d_c.get(), d_s.get(), eps, d_scan.get(), d_pts.get(), d_err.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(scan, d_scan.get(), n * 8, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(points, d_pts.get(), n * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&herr, d_err.get(), 4, hipMemcpyDeviceToHost));
    if (herr) return fail(FTGP_ERR_ARG, "fakelidar: IndexError (a ray left the image through the right or bottom edge)%s");
    return 0;
}

int ftgp_last_kernel_ms(FtgpEnv* e, float* ms)
{
    if (!e || !ms) return fail(FTGP_ERR_ARG, "null argument%s");
    if (!e->timed) return fail(FTGP_ERR_STATE, "no step/rollout has been launched yet%s");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(e->ev_stop[e->cur_slot].get()));
    HIP_TRY(hipEventElapsedTime(ms, e->ev_start.get(), e->ev_stop[e->cur_slot].get()));
    return 0;
}

// diagnostic libraries only (-DFTGP_DIAG, csrc/diag/ftgp_diag.inc): read and clear the phase stamps, workgroup tables
#if defined(FTGP_DIAG) && defined(FTGP_STAMPS)
int ftgp_debug_stamps(unsigned long long* out)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ftgp_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    unsigned long long z[16] = { 0 };
    return hipMemcpyToSymbol(HIP_SYMBOL(ftgp_stamps), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
#if defined(FTGP_DIAG) && defined(FTGP_STAMPS)
int ftgp_debug_substamps(unsigned long long* out)          // read and clear
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ftgp_substamps), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    unsigned long long z[32] = { 0 };
    return hipMemcpyToSymbol(HIP_SYMBOL(ftgp_substamps), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
#if defined(FTGP_DIAG) && defined(FTGP_WG_TIMES)
int ftgp_debug_set_wg_groups(const int* groups, int n_blocks)      // groups == nullptr: identity
{
    std::vector<int> g(8192, 0);
    if (groups) { for (int i = 0; i < n_blocks && i < 8191; ++i) g[i] = groups[i]; g[8191] = 1; }
    return hipMemcpyToSymbol(HIP_SYMBOL(ftgp_wg_group), g.data(), sizeof(int) * 8192) == hipSuccess ? 0 : -1;
}
int ftgp_debug_wg_times(unsigned long long* out, int n_blocks)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ftgp_wg_times), sizeof(unsigned long long) * 4 * (size_t)n_blocks) == hipSuccess ? 0 : -1;
}
#endif

// What this library was built from and with: "abi=<n> sources=<hash> diag=<switches|none> fair_shift=<n> waves_per_eu=<n>".  The hash is
// tools/evidence.py's hash of the kernel sources, handed in by the build (__graft_entry__.build: -DFTGP_BUILD_SOURCES=...); a library
// built by hand without it says "unstamped".  Touches no device.
#ifndef FTGP_BUILD_SOURCES
#define FTGP_BUILD_SOURCES unstamped
#endif
#define FTGP_STR2_(x) #x
#define FTGP_STR_(x) FTGP_STR2_(x)
const char* ftgp_build_info(void)
{
    return "abi=" FTGP_STR_(FTGP_ABI_VERSION) " sources=" FTGP_STR_(FTGP_BUILD_SOURCES) " diag=" FTGP_DIAG_FLAGS
           " fair_shift=" FTGP_STR_(FTGP_FAIR_SHIFT) " waves_per_eu=" FTGP_STR_(FTGP_WAVES_PER_EU);
}

int ftgp_selftest(int device_id, int64_t* mismatches)
{
    if (!mismatches) return fail(FTGP_ERR_ARG, "null argument%s");
    if (int rc = open_device(device_id)) return rc;
    DevBuf<unsigned long long> d; unsigned long long h = 0;
    HIP_TRY(dev_alloc(d, sizeof h));
    hipError_t e1 = hipMemset(d.get(), 0, sizeof h);
    hipLaunchKernelGGL(ftgp_selftest_rcp_kernel, dim3(1u << 12), dim3(256), 0, 0, d.get());
    hipError_t e2 = hipGetLastError();
    hipError_t e3 = hipMemcpy(&h, d.get(), sizeof h, hipMemcpyDeviceToHost);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(FTGP_ERR_HIP, "selftest: HIP error%s");
    *mismatches = (int64_t)h;
    return 0;
}

const char* ftgp_kernel_name(FtgpEnv* e)
{
    if (!e) return "ftgp_step_kernel";
    return step_kernel(e, e->last_roster, e->last_net).name;      // the instantiation of the newest launch (before any: the single-driver one)
}

}  // extern "C"
