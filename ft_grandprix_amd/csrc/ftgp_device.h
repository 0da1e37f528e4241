// ftgp_device.h -- device-side state layout and wave-level helpers (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/ftgp.h"
#include "ftgp_march.h"
#include "ftgp_spawn.h"
#include "ftgp_net.h"
#include "ftgp_frame.h"
#include "ftgp_rival.h"

#define FTGP_WAVE 64
#define FTGP_MAX_GROUPS 256              // groups of 64 rays per car: n_rays <= 16384
#define FTGP_TASK_MASKED (1 << 25)       // window-only table, word [0] of a draw: not a plain draw (DeviceParams::task_tab)
#define FTGP_MAX_CARS_PER_BLOCK 16      // K1 / K3 run one car per lane group of a single wave: 16 cars x 4 lanes

// Per-car state, array-of-structs in HBM.  The step kernel keeps CarCore in LDS for the whole launch.
struct alignas(16) CarCore {
    double x, y, qw, qz;          // planar pose (yaw as quaternion (qw, 0, 0, qz))
    double vx, vy, wz;            // world-frame linear velocity, yaw rate
    double qs, qsd;               // virtual steering joint
    double w[4];                  // wheel spin fl, fr, bl, br
    double u_speed, u_steer;      // controls
    double last_steer;            // fast.py:12
    double dist2;                 // squared distance to the centre-line (custom.py:1343)
    int32_t completion, laps, offset, n_times;
    int32_t good_start, finished, off_track, delta;
    int64_t start;                // env step of the last counted line crossing (vehicle_state.start, custom.py:1362): 64 bits like self.steps
    int64_t finish_step;          // env step at which `finished` was set (custom.py:1367-1370); meaningful while finished != 0
};
// The lap-time list stays in HBM (written on lap crossings only).
struct alignas(16) CarState : CarCore {
    double times[FTGP_MAX_LAP_TIMES];
};
static_assert(sizeof(CarCore) == 192 && offsetof(CarCore, finish_step) == offsetof(CarCore, start) + 8, "CarCore layout (progress_update reaches finish_step through &start)");
static_assert(sizeof(CarState) == 192 + 8 * FTGP_MAX_LAP_TIMES, "CarState layout");
static_assert((FTGP_MAX_LAP_TIMES & (FTGP_MAX_LAP_TIMES - 1)) == 0, "the lap-time ring is indexed with a mask");

// LiDAR frame of one car, refreshed in LDS before every sweep: the sweep never reads the live state, so the dynamics
// of the same step can run beside it.  The second half is what OTHER cars of the env need to see this car.
struct alignas(16) LidarFrame {
    float u0, v0, chf, shf;       // LiDAR centre in pixels (binary32 of the binary64 value), heading (cos, sin) in binary32
    double lcx, lcy;              // LiDAR centre, world                         } FTGP_LIDAR_FAKELIDAR: i_x, i_y = the car's position in pixels
    double x, y, qw, qz;          // pre-step pose                               } (custom.py:1382-1384) and x, y = heading (cos, sin) instead
    int32_t finished;
    int32_t slot0;                // first car slot (inside the workgroup) of this car's env      } multi-car envs only:
    float fx, fy;                 // binary32 of x, y: what the inter-vehicle cull compares        } see frame_write()
};
static_assert(sizeof(LidarFrame) == 80, "LidarFrame layout");

// Multi-car envs: what a ray of car `me` needs to know about env-mate k to rule it out without looking at it.  B = mate's
// origin - my LiDAR centre; every visible part of the mate lies within `cull` of its origin, so a ray of direction d can only
// touch it if the mate sits in front and within `cull` of the ray's line, i.e. if  B . d >= sqrt(|B|^2 - cull^2) =: t.
// t = +inf: never (myself, a finished car -- invisible, custom.py:1441-1466 -- or my own rangefinders are off);
// t = -inf: always look (the mate is closer than 2 cull + ring radius, where the bound does not hold).
struct alignas(16) PairCull { float bx, by, t, pad; };
#define FTGP_PAIR_STRIDE 8              // FtgpConfig.cars_per_env <= 8

struct DeviceParams {
    // sizes
    int32_t n_envs, cars_per_env, n_cars, n_rays;
    int32_t lap_target, spawn_mode, ranges_stride, env_base;
    uint64_t seed;
    double dt;
    double rpp;                   // radians per LiDAR point, (2 pi) / n_rays (nidc.py:121), divided once on the host
    float two_over_rpp, pad_f0;   // 2 / rpp in binary32: seeds the cover-count search (cover_count), nothing else
    // track
    int32_t width, height, words_per_row, fstride;      // fstride = width + 2: cells per row of a field plane (one-pixel ring)
    double px_size_x, px_size_y, origin_x, origin_y, inv_px_x, inv_px_y;
    float inv_px_x_f, inv_px_y_f;
    float snap_eps;               // the march re-checks a landing point with the exact comparisons within this distance of a pixel boundary
    uint32_t dyn_table_lo;        // per-car dynamics (ftgp_set_dynamics): the low half of the records' device address, 0 until the first setter call (dyn_table())
    uint32_t plane256;            // bytes per (padded) sector plane of the box field / 256
    int32_t n_sectors;            // direction sectors of this handle's box field: 8 x (1, 2, 4 or 8 slope slices per octant)
    float slice_factor;           // FTGP_SLICE_FACTOR(FTGP_SLOPE_SLICES): a ray's sector is found among all FTGP_SECTORS, sector_tab maps it to planes
    int32_t n_planes;             // planes of the field (= n_sectors)
    uint32_t net_table_lo;        // network drivers (ftgp_set_net): the low half of the NetDev table's device address, 0 until the first setter call (net_table())
    int32_t contact_reach;        // chessboard reach (pixels) of the wall-contact window; `nearbits` is the wall set dilated by it
    // step-kernel launch shape and LDS layout (byte offsets, all 16-B aligned)
    int32_t cars_per_block, waves_per_block, eighth, win_floats;   // win_floats: floats per LDS scan row: (eighth % 4) + (n_rays - 2*eighth) + 1, padded to 4
    int32_t off_params, off_veh, off_path, off_ray, off_cars, off_frame, off_steps, off_scan, off_list, off_pool, off_k1, off_cover, lds_bytes, cover_kmax;
    int32_t off_mmask, mmask_stride;      // multi-car envs: [2][cars_per_block][mmask_stride] bytes, which env-mates a ray group can see (mate_masks)
    int32_t bubble_wrap;          // custom.py:1041-1055: the four wheel softeners collide with the walls
    int32_t n_cu;                 // compute units of the device (sweep_priority)
    uint32_t net_table_hi;        // ... and its high half (two words that were spare: the block's layout is what it was)
    float edge_margin, pad_d;     // pixels: a LiDAR centre at least this far from every image edge has all its ray origins on the image (frame_write)
    // FTGP_LIDAR_FAKELIDAR (raycast.py:5-21 inside the step loop): the distance transform, the binary64 fan and the world size of the map
    const double* edt;            // [height][width] exact Euclidean distance to the nearest wall pixel (0 on walls), pixels; null in RANGEFINDER mode
    const double* fan_dirs;       // [n_rays][2] body-frame fan directions, binary64
    double map_size;              // 20 * scale = 40 (custom.py:1382)
    int32_t lidar_mode;
    int32_t win_tasks_per_car;    // tasks per car of the window-only table (task_tab's third); 0: FTGP_SCAN_EVERY_STEP, every step sweeps and stores every ray (a word that was spare)
    int32_t tasks_per_car;        // the sweep's work list per car (lidar_groups): groups of 64 consecutive rays, or pairs of opposite groups
    float group_cg, group_sg;     // cos / sin of the half-width of a ray group as mate_masks() needs it (cg < -1: no bound, e.g. a caller's fan)
    uint32_t dyn_table_hi;        // ... and its high half (two words that were spare: the block's layout is what it was)
    const uint16_t* field;        // [n_sectors][height + 2][width + 2] box entries (ftgp_march.h), HBM/L2
    const uint32_t* bits;         // [height][words_per_row] wall bitmap
    const uint32_t* nearbits;     // [height][words_per_row] wall bitmap dilated by contact_reach (early-out of the wall contact)
    const void* veh_dev;          // VehLds image (vehicle constants + wheel loads) in HBM
    const double* path;           // [100][2]
    const double* spawn;          // [100][4] x, y, qw, qz
    const float* ray_dir;         // [n_rays][2] body-frame ray directions (sin phi, -cos phi), binary32
    const float* cover_thr;       // [2][cover_kmax + 1 (padded to 4)] cover-count thresholds of the nidc / fast drivers (cover_count)
    // state
    CarState* cars;
    float* ranges;                // [n_cars][ranges_stride]
    int64_t* steps;               // [n_envs]
    // end-of-launch metrics (ftgp_step_kernel's epilogue): one FTGP_METRIC_DOUBLES record per workgroup, an arrival counter, and
    // the two places the last workgroup to arrive writes the launch's record to (device memory for the RCCL all-gather, pinned
    // host memory for the caller); null: the step kernel leaves the metrics to ftgp_metrics_kernel
    double* wg_metrics;
    unsigned int* wg_ticket;
    double* metrics_dev;          // [2][FTGP_METRIC_DOUBLES]: the launch's slot (a kernel argument, alternating per launch) says which
    double* metrics_host;         // [2][FTGP_METRIC_DOUBLES]
    double* wg_metrics_host;      // [2][workgroups][FTGP_METRIC_DOUBLES] pinned host memory: the partial records of a launch whose record nothing on the device
                                  // needs (one rank, no communicator) -- the host adds them up
    alignas(16) int32_t sector_tab[FTGP_SECTORS][4];     // ftgp_sector_entry() of every sector (staged into LDS with the head of the block)
    FtgpVehicle veh;              // host-side copy (the step kernel reads the LDS image VehLds; from here on nothing is staged into LDS)
    double wheel_load[4];
    const unsigned char* stage_img;      // what every workgroup stages at the start of a launch, in ONE pass: the image of the LDS bytes [off_params, off_cars)
                                  // (head of this block | VehLds | path | fan), then the cover tables of nidc and of fast, stage_cover bytes each
    int32_t stage_cover, reserved3;
    int32_t car_policy[FTGP_MAX_CARS_PER_BLOCK];       // FTGP_POLICY_PER_CAR: the driver of the workgroup's car slot c (= the roster's entry c % cars_per_env: a workgroup
                                  // holds whole envs); 0 = not set.  Read with scalar loads.
    int32_t group_order[FTGP_MAX_GROUPS];      // the tasks of a car by expected march length, longest first (rays along the car's axis look down the
                                  // track, sideways rays hit the corridor wall at once): first ray | kind << 16, kind 0 = one group of 64
                                  // consecutive rays, 1 = that group and the opposite one (first ray + n/2), 2 = the short ends of both halves in
                                  // one group (lanes 0..31 / 32..63); read with scalar loads
    int32_t win_group_order[FTGP_MAX_GROUPS];  // right behind it, the window-only list's tasks in its order (plan_window_table), as group_order holds the first
                                  // table's; kind 3, a gather: lanes | gather number << 7 in the low half (mate_masks looks at every mate for it, as for kind 2)
    const int32_t* task_tab;      // [2][cars_per_block * tasks_per_car][4] the sweep's draws, one 16-byte scalar load each (lidar_groups; behind this block in device memory):
                                  //   [0] first ray (14 bits) | kind << 14 | car slot << 16 | window class of the first / second group << 20 / 22 | (the first group holds ray 0) << 24
                                  //       (window class: 0 = no ray of the group lies in the drivers' scan window, 1 = every ray does, 2 = test per ray)
                                  //   [1] byte offset of the car's LidarFrame in a frame buffer | rank of the task among the car's << 16
                                  //   [2] byte offset of the car's row of ranges from the workgroup's first row
                                  //   [3] byte offset, in a scan buffer, at which sample j of the car sits when 4 j is added: row + ((eighth & 3) - eighth) floats
                                  // the second table is for launches whose drivers do not read the scan: window classes 0, no ray 0
                                  // Behind the two, [cars_per_block * win_tasks_per_car][4]: the window-only table, for every step but the last of a launch whose
                                  // drivers read the scan -- the rays the drivers read (ranges[0], ranges[eighth : n - eighth]) and no other, in a cut and an
                                  // order of their own (plan_window_table, win_group_order): pairs and single groups of 64 live rays each, first ray anywhere,
                                  // window class 1, and
                                  //   kind 3, a GATHER: [0]'s first-ray field holds lanes (7 bits) | gather number << 7; lane l < lanes marches ray l + d of the
                                  //   run it lies in, window class 2 (a test per ray), the ray-0 flag where a run is ray 0.  The rank in [1] is the task's in
                                  //   win_group_order; [2], [3] as in the first table.
                                  //   FTGP_TASK_MASKED in [0]: the draw is not a plain one.  A PLAIN draw -- kind 0 or 1, 64 live rays per group, every group
                                  //   wholly inside the window, no ray 0 -- runs through the window-only sweep without a lane mask and without a delivery test
                                  //   (lidar_groups): the bit is set on every gather, and on every entry where this table is the first table again.
                                  // Behind those draws, [gathers][4]: the runs of each gather task, in lane order, one word each: (first ray - first lane) & 0xffff |
                                  // first lane << 16; a run the task does not have starts at lane 64.  The same for every car slot.
};

static_assert(offsetof(DeviceParams, win_group_order) == offsetof(DeviceParams, group_order) + sizeof(int32_t) * FTGP_MAX_GROUPS, "win_group_order lies right behind group_order (dynamics_lanes)");

// Bytes of one parameter block in device memory.  Multi-track handles (ftgp_create_tracks): the workgroup table follows track 0's block,
// int4 per workgroup = (byte offset of its track's block from track 0's, first car, number of cars, track).
#define FTGP_PARAMS_BYTES ((sizeof(DeviceParams) + 15) & ~(size_t)15)

// vehicle constants as staged into LDS
struct VehLds {
    FtgpVehicle v;
    double wheel_load[4];
    float cull_radius;            // every part of a car that a ray can see lies within this distance of the car's origin
    int32_t puck_in_box;          // the LiDAR puck's disc lies inside the chassis box by a margin above what the cancellation in the circle's discriminant can move the puck at the far end of the map (plan_vehicle): a ray then meets the box no later than
                                  // the puck, min(box, puck) is the box's time to the bit, and ray_vs_car() leaves the circle test (a square root) out
    // binary32 of the constants the inter-vehicle ray test uses (the conversions the specification makes per test, made once)
    float box_xmin_f, box_xmax_f, box_ymin_f, box_ymax_f, lidar_x_f, lidar_y_f, ring_radius_f, pad_f;
};

// Per-car dynamics (ftgp_set_dynamics): one record of FTGP_DYN_RECORD doubles per car in HBM, allocated by the first setter call: the
// eight entries of the car's row in the header's order, then its four static wheel loads; behind the records, the counter of rejected
// rows.  The parameter blocks carry the address in two spare words (dyn_table_lo / _hi), so their layout, the staging image and the LDS
// offsets are what they were.  A step launch with the table on stages its workgroup's records into LDS behind the layout of
// lds_layout(), at lds_bytes (ftgp_step_kernel<..., DYN = true>).
// (FTGP_DYN_RECORD = 12: include/ftgp.h, where the env-state record documents it)
enum { kDynMass = 0, kDynIzz, kDynFriction, kDynTireDamping, kDynThrottleKv, kDynThrottleForceLimit, kDynSteerKp, kDynSteerDamping, kDynWheelLoad };
template <class PP> __host__ __device__ inline double* dyn_table(PP p) { return reinterpret_cast<double*>(((uint64_t)p->dyn_table_hi << 32) | (uint64_t)p->dyn_table_lo); }
template <class PP> __host__ __device__ inline unsigned long long* dyn_rejected(PP p) { return reinterpret_cast<unsigned long long*>(dyn_table(p) + (size_t)p->n_cars * FTGP_DYN_RECORD); }
#define FTGP_DYN_BYTES(n_cars) ((size_t)(n_cars) * FTGP_DYN_RECORD * sizeof(double) + 16)
// ftgp_dynamics_kernel's arguments: the handle's own row and what turns a mass into wheel loads (plan()'s static wheel loads: load[r] =
// wtot * load_k[r], halved where load_half[r])
struct DynArgs {
    double base[FTGP_DYN_DOUBLES];
    double gravity, load_k[4];
    int32_t load_half[4];
    int32_t init, pad;                // init: the table is being turned on -- every car's record starts as the handle's own
    const double* rows;               // [n_cars][FTGP_DYN_DOUBLES] or null
    const uint8_t* env_mask;          // [n_envs] or null = all envs
    const uint8_t* env_mask_or;       // [n_envs] or null: with env_mask, an env is taken if either byte is set (ftgp_collect_device: terminated | truncated)
};

// Network drivers (ftgp_set_net): FTGP_MAX_NETS records in HBM, allocated by the first setter call; the parameter blocks carry the
// table's address in two spare words (net_table_lo / _hi), as with the dynamics table.  A record is the description as the kernel reads
// it (scalar loads) and the address of the slot's parameters in the LIBRARY's layout: per layer the weights transposed and padded,
// Wt[n_in][ld] with ld = n_out rounded up to 64 (the padding is zeros), then b[ld] -- lane j of a wave owns neurons j and j + 64, and the
// wave's load of row k is one or two coalesced 256-byte segments that every car shares through L2.
struct alignas(16) NetDev {
    int32_t defined, pool, beam_first, n_beams, use_state, n_layers, hidden_act, out_act;
    int32_t width[FTGP_NET_MAX_LAYERS + 1];       // width[0] = n_in, width[l + 1] = outputs of layer l
    int32_t w_off[FTGP_NET_MAX_LAYERS], b_off[FTGP_NET_MAX_LAYERS];      // float offsets of Wt and b of layer l in params
    int32_t n_floats;                             // floats of the slot's buffer in the library's layout
    int32_t frame_first, frame_shape;             // frame inputs (ftgp_set_net_frame; the two words that were spare): the index of the first one, and
                                                  // n_ahead | stride << 8 -- 0 = none, as ftgp_set_net leaves it (an enabled frame has stride >= 1)
    float max_range, inv_max_range, out_scale[2], out_offset[2];
    const float* params;
    int32_t rival_first, rival_shape;             // rival inputs (ftgp_set_net_rivals): the index of the first one, and enabled | n_rivals << 8 -- 0 = none
    const int32_t* env_member;                    // a population (ftgp_set_net_population; the eight bytes that were spare): [n_envs] the member of
                                                  // every env, and params is then [n_members] sets, net_member_stride(n_floats) floats apart; null = none
};
static_assert(sizeof(NetDev) == 144 && offsetof(NetDev, env_member) == 136, "NetDev layout");
// floats from one member's parameters to the next in a population: the slot's n_floats rounded up to 64 floats, a whole 256-byte segment
__host__ __device__ inline int net_member_stride(int n_floats) { return ftgp_net_member_stride(n_floats); }
template <class PP> __host__ __device__ inline const NetDev* net_table(PP p) { return reinterpret_cast<const NetDev*>(((uint64_t)p->net_table_hi << 32) | (uint64_t)p->net_table_lo); }
__host__ __device__ inline bool is_net_policy(int policy) { return policy >= FTGP_POLICY_NET0 && policy <= FTGP_POLICY_NET3; }

// ---------------------------------------------------------------------------------------------
// Specified polynomials (DESIGN.md "arithmetic rules"): Taylor series in Horner form on x*x.
// Written operation by operation; the library is compiled with -ffp-contract=off.
__device__ __forceinline__ double spec_sin(double x)
{
    double z = x * x;
    double p = -1.0 / 51090942171709440000.0;
    p = p * z + 1.0 / 121645100408832000.0;
    p = p * z - 1.0 / 355687428096000.0;
    p = p * z + 1.0 / 1307674368000.0;
    p = p * z - 1.0 / 6227020800.0;
    p = p * z + 1.0 / 39916800.0;
    p = p * z - 1.0 / 362880.0;
    p = p * z + 1.0 / 5040.0;
    p = p * z - 1.0 / 120.0;
    p = p * z + 1.0 / 6.0;
    p = p * z;
    return x - x * p;
}
__device__ __forceinline__ double spec_cos(double x)
{
    double z = x * x;
    double p = 1.0 / 2432902008176640000.0;
    p = p * z - 1.0 / 6402373705728000.0;
    p = p * z + 1.0 / 20922789888000.0;
    p = p * z - 1.0 / 87178291200.0;
    p = p * z + 1.0 / 479001600.0;
    p = p * z - 1.0 / 3628800.0;
    p = p * z + 1.0 / 40320.0;
    p = p * z - 1.0 / 720.0;
    p = p * z + 1.0 / 24.0;
    p = p * z - 0.5;
    p = p * z;
    return 1.0 + p;
}

// splitmix64 / u01, the counter-based generator: ftgp_spawn.h

// ---------------------------------------------------------------------------------------------
// wave64 helpers
// (from the hardware's lane counters, not from threadIdx.x: the thread index then need not be kept in a register -- or in scratch
// memory -- for the whole life of a persistent kernel)
__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ double shfl_xor_f64(double v, int m)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, m, FTGP_WAVE);
    hi = __shfl_xor(hi, m, FTGP_WAVE);
    return __hiloint2double(hi, lo);
}

// wave-uniform values pinned in SGPRs (values read from LDS arrive in VGPRs even when every lane reads the same address)
__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float sgpr(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// wave-uniform copy of a pointer that was read from LDS (keeps it in SGPRs: global_load with an SGPR base)
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<T*>(((uint64_t)hi << 32) | lo);
}

// Orders this wave's LDS stores before its later LDS loads (lanes exchange data through LDS without a
// workgroup barrier: DS operations of one wave execute in order, the fence keeps the compiler honest).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
