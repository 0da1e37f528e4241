/*
 * ftgp.h -- C-ABI of the MI355X-native ft_grandprix hot path
 *           (vehicle integrate + LiDAR sweep + lap progress, batched over envs).
 *
 * This is the drop-in boundary.  The reference has no FFI:
 * its hot loop talks to MuJoCo's Python bindings.  Each entry point below names
 * the reference call sites it replaces (paths relative to the reference repo).
 *
 * Conventions: extern "C", opaque handle, int status (0 = ok, negative = error,
 * text via ftgp_last_error()), plain pointers and sizes only.  The caller owns
 * all host buffers; device buffers are owned by the handle.  A handle is not
 * thread-safe; independent handles are.
 *
 * Layout conventions for per-car arrays: index = (env * cars_per_env + car).
 */
#ifndef FTGP_H
#define FTGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTGP_ABI_VERSION 5

/* status codes */
#define FTGP_OK              0
#define FTGP_ERR_ARG        -1   /* bad argument / config */
#define FTGP_ERR_NO_DEVICE  -2   /* no HIP device (the product path has no CPU fallback) */
#define FTGP_ERR_HIP        -3   /* HIP runtime error */
#define FTGP_ERR_STATE      -4   /* call not valid in the handle's current state */
#define FTGP_ERR_COMM       -5   /* RCCL error */

/* device-side policies for ftgp_rollout; FTGP_POLICY_HOST = ctrl comes from ftgp_set_ctrl */
#define FTGP_POLICY_HOST      0
#define FTGP_POLICY_LOBOTOMY  1  /* ft_grandprix/lobotomy.py:2-3 : (0, 0)                    */
#define FTGP_POLICY_NIDC      2  /* ft_grandprix/nidc.py:116-131 : disparity extender         */
#define FTGP_POLICY_FAST      3  /* ft_grandprix/fast.py:118-139 : same + straight-line boost */
#define FTGP_POLICY_RANDOM    4  /* counter-based RNG keyed (seed, car, step): speed~U(0,3), steer~U(-1,1) */
#define FTGP_POLICY_PER_CAR   5  /* every car slot of an env its own driver, as set by ftgp_set_car_policies (the roster) */
/* 6 .. 9: FTGP_POLICY_NET0 .. FTGP_POLICY_NET3, the network drivers (ftgp_set_net, below) */

#define FTGP_VEHICLE_MUSHR     0
#define FTGP_VEHICLE_TRICYCLE  1

/* what the rangefinders are (FtgpConfig.lidar_mode) */
#define FTGP_LIDAR_RANGEFINDER 0  /* exact 2-D ray against the wall pixels and the other cars (template/mushr.em.xml:112-117,204-206 as read at
                                     custom.py:1395) */
#define FTGP_LIDAR_FAKELIDAR   1  /* the reference's own 2-D LiDAR: sphere tracing over the Euclidean distance transform of the track image,
                                     ft_grandprix/raycast.py:5-21, wired as custom.py:1381-1393 (option use_simulated_simulation_lidar) */

#define FTGP_PATH_POINTS   100   /* ft_grandprix/curve.py:8 */
#define FTGP_MAX_LAP_TIMES  32   /* lap times kept per car: a ring of the NEWEST 32 -- lap time number k (0-based, in the order VehicleState.times
                                    lists them, custom.py:124,1351-1363) sits in slot k % 32; the true count is kept beside it.  VehicleState.times
                                    is unbounded; lap_target defaults to 10 (custom.py:961).  A backward crossing pops the newest entry (custom.py:1355-1356):
                                    while more than 32 lap times have been counted, the popped entry had overwritten the oldest one the list would
                                    still show -- that slot then reads NaN (= no entry; skipped by the metrics record's min / max) until it is filled again */

/* number of doubles / ints per car in the packed read-back rows */
#define FTGP_SNAPSHOT_DOUBLES 10 /* laps, vel[3], yaw, pitch, roll, lap_completion, absolute_completion, time */
#define FTGP_POSE_DOUBLES     13 /* qpos[7] = x y z qw qx qy qz ; qvel[6] = vx vy vz wx wy wz */
#define FTGP_PROGRESS_INTS    10 /* laps, completion, lap_completion, absolute_completion, finished, off_track, start, good_start, delta,
                                    finish_step: the env step at which `finished` was set (custom.py:1367-1370), -1 while racing;
                                    the row is int32 while steps are int64: saturates at 2^31 - 1 (99 days of simulated time) */
#define FTGP_METRIC_DOUBLES    8 /* steps, n_cars, sum_laps, sum_abs_completion, n_finished, n_off_track, min_lap_time, max_lap_time */

/*
 * Track geometry (built by ft_grandprix_amd/track.py from <track>.png + <track>-path.svg).
 *   wall bitmap : ft_grandprix/chunk.py:39-43 threshold (wall iff pure white)
 *   wall frame  : template/mushr.em.xml:17-20,55,92 (pixel (px,py) covers
 *                 x in [origin_x + px*px_size_x, +px_size_x), y in (origin_y - (py+1)*px_size_y, origin_y - py*px_size_y])
 *   path        : ft_grandprix/curve.py:6-18 + ft_grandprix/custom.py:1184-1186 (100 x (x, y), float64)
 */
typedef struct FtgpTrack {
    int32_t width, height;          /* pixels */
    int32_t words_per_row;          /* uint32 words per bitmap row = ceil(width/32) */
    int32_t reserved0;
    const uint32_t *bits;           /* [height][words_per_row]; bit (x & 31) of word (x >> 5), 1 = wall */
    double px_size_x, px_size_y;    /* world units per pixel */
    double origin_x, origin_y;      /* world position of the top-left corner of pixel (0, 0) */
    const double *path;             /* [FTGP_PATH_POINTS][2] world coordinates */
} FtgpTrack;

/*
 * Vehicle parameters: the reduced planar model of the MuSHR car of
 * template/mushr.em.xml:61-89,95-198 (see DESIGN.md "K1").  ftgp_default_vehicle() fills
 * the values lifted from that file.
 */
typedef struct FtgpVehicle {
    double mass, izz;               /* total mass, yaw inertia about the CoM */
    double wheel_x[4], wheel_y[4];  /* fl, fr, bl, br contact points, body frame (mushr.em.xml:124,137,150,162) */
    double wheel_radius;            /* 0.03 (mushr.em.xml:24,69) */
    double wheel_inertia;           /* spin inertia incl. armature 0.01 (mushr.em.xml:81) */
    double wheel_damping;           /* 0.01 (mushr.em.xml:81) */
    double throttle_kv, throttle_gear, throttle_force_limit; /* 100, 0.04, 500 (mushr.em.xml:180) */
    double steer_kp, steer_damping, steer_inertia, steer_limit; /* 20, 3*0.1, ~8e-4, 1 rad (mushr.em.xml:78,179) */
    double friction, gravity;       /* 0.5 = max(wheel 0.3, plane 0.5) (mushr.em.xml:69,94); 9.81 */
    double tire_damping;            /* slip-velocity coupling per wheel, N s/m (from solref 0.02/solimp 0.95, mushr.em.xml:69) */
    double contact_x[3];            /* body-frame x of the 3 wall/car contact circles */
    double contact_radius;
    double contact_stiffness, contact_damping; /* penalty spring/damper against walls and other cars */
    double lidar_x, lidar_y;        /* LiDAR centre, body frame: (-0.0525, 0) (mushr.em.xml:101) */
    double lidar_ring_radius;       /* 0.03: ray j starts at centre - 0.03*dir_j (mushr.em.xml:103,115) */
    double body_z;                  /* constant ride height reported in qpos[2] */
    double box_xmin, box_xmax, box_ymin, box_ymax; /* chassis bbox, body frame, seen by other cars' rays */
    double softener_radius;         /* bubble_wrap: wall-contact circles at the four wheel positions; 0.65 * 0.0488 = radius of
                                       meshes/mushr_wheel.stl at the scale of mushr.em.xml:39 (softener geoms, mushr.em.xml:65-67) */
    double motor_forward_limit, motor_turn_limit; /* FTGP_VEHICLE_TRICYCLE: ctrlrange of the two torque motors (car.em.xml:138-139) */
    int32_t kind;                   /* FTGP_VEHICLE_MUSHR: Ackermann car with a velocity servo and a steering servo (mushr.em.xml);
                                       FTGP_VEHICLE_TRICYCLE: the legacy differential-drive car of template/car.em.xml (option tricycle_mode,
                                       custom.py:1154-1170): wheels 0 / 1 = left / right driven wheels, wheel 2 = frictionless front caster,
                                       ctrl = (forward torque, turn torque) on the tendons 0.5 (l + r) and 0.5 (r - l) (car.em.xml:126-139) */
    int32_t reserved1;
} FtgpVehicle;

typedef struct FtgpConfig {
    int32_t abi_version;            /* FTGP_ABI_VERSION */
    int32_t n_envs;
    int32_t cars_per_env;           /* 1..8; cars of one env share a world (template/cars/cars.json) */
    int32_t n_rays;                 /* rangefinders per car (custom.py:1158 uses 90; BASELINE uses 1080) */
    int32_t lap_target;             /* custom.py:961, used custom.py:1367 */
    int32_t device_id;              /* HIP device ordinal */
    int32_t spawn_mode;             /* 0 = reference: car i at path[(i+5)*2] (custom.py:1112,1232-1245);
                                       1 = benchmark spread: global env e, car i at path[(10 + 7*e + 2*i) % 98] with seeded yaw jitter */
    int32_t env_base;               /* global index of this handle's env 0: a shard [env_base, env_base + n_envs) of a larger batch spawns,
                                       jitters and draws random controls exactly like the same slice of the monolithic batch */
    uint64_t seed;                  /* spawn jitter and FTGP_POLICY_RANDOM */
    double dt;                      /* 0.004 (mushr.em.xml:30) */
    int32_t bubble_wrap;            /* option "bubble_wrap" (custom.py:970,1041-1055): the four wheel softeners (mushr.em.xml:65-67,126-129)
                                       collide with the walls -- here: four more wall-contact circles at the wheel positions */
    int32_t naive_flatten;          /* option "naive_flatten" (custom.py:981,1338-1339): re-projects the body quaternion onto pure yaw every
                                       step; the planar model has no pitch / roll, so this is accepted and changes nothing */
    int32_t lidar_mode;             /* FTGP_LIDAR_RANGEFINDER (default) or FTGP_LIDAR_FAKELIDAR (option "use_simulated_simulation_lidar",
                                       custom.py:987,1381-1393).  FAKELIDAR, per car and step, in binary64:
                                         origin   i_x = (x / map_size) * width, i_y = -(y / map_size) * height of the car's position (custom.py:1382-1384)
                                         ray j    image-frame direction (dxw, -dyw), (dxw, dyw) = R(yaw) * fan_dirs[j] -- ray order and orientation
                                                  as the rangefinders' (index 0 = rear, counter-clockwise; the dead branch's own linspace,
                                                  custom.py:1387, was never exercised: SURVEY.md 8a-3)
                                         march    raycast.py:5-21 on the exact Euclidean distance transform of the wall image (the recipe of
                                                  custom.py:1149-1153 / raycast.py:24-27, built at ftgp_create: integer squared distances, one sqrt)
                                         range    (scan / width) * map_size (custom.py:1392-1393), stored as binary32
                                       int() truncates toward zero and negative indices wrap like numpy's: an index is valid iff -width <= int(x) < width
                                       and -height <= int(y) < height.  A lookup past the right / bottom edge, or below -width / -height -- the reference's
                                       IndexError either way -- ends the ray with range -1, whatever it had accumulated.  A ray whose lookup was valid
                                       ends without error, with the distance it has, once x < 0 or y < 0 (the loop condition, tested after the lookup).
                                       The rays see walls only (no other cars), as there. */
    int32_t reserved2;
    double map_size;                /* FAKELIDAR: world size of the map, 20 * scale = 40 (custom.py:1155,1382; mushr.em.xml:16-18); <= 0 means 40 */
    const double *fan_dirs;         /* optional [n_rays][2]: body-frame unit directions of the rangefinder fan; NULL = the sites of
                                       template/mushr.em.xml:112-117, (sin phi_j, -cos phi_j) with phi_j = radians(360 / n_rays * j - 90).
                                       FAKELIDAR mode uses the binary64 values as they are.  RANGEFINDER mode uses their binary32 roundings -- for
                                       fan_dirs == NULL and an even n_rays with the second half of the table written as the exact negation of the
                                       first (site j + n/2 looks exactly opposite to site j: the sweep derives a ray from its opposite); a caller's
                                       fan is rounded entry by entry. */
    FtgpTrack track;
    FtgpVehicle vehicle;
} FtgpConfig;

typedef struct FtgpEnv FtgpEnv;

/* Fill *v with the MuSHR constants of template/mushr.em.xml. */
void ftgp_default_vehicle(FtgpVehicle *v);

/* Fill *v with the constants of the legacy tricycle of template/car.em.xml (use FtgpConfig.dt = 0.0075, car.em.xml:11). */
void ftgp_tricycle_vehicle(FtgpVehicle *v);

/* Text of the last error raised on the calling thread. */
const char *ftgp_last_error(void);

/* Number of visible HIP devices (<= 0 when there is none). */
int ftgp_device_count(void);

/*
 * Build the world.  Replaces Mujoco.stage(): chunk() + produce_mjcf() + MjModel.from_xml_path +
 * MjData + path load (ft_grandprix/custom.py:1133-1194; drive.py:21-46).  Uploads the track,
 * builds the ray-march acceleration grid, allocates per-car state and calls ftgp_reset(NULL).
 */
int ftgp_create(const FtgpConfig *cfg, FtgpEnv **out);
int ftgp_destroy(FtgpEnv *env);

/*
 * Multi-track batches: several worlds of one handle, each on its own track, stepped by one launch.  The reference builds one world per
 * track: its GUI lists every PNG of the template directory (custom.py:879-887) and stage() rebuilds the world on the one picked
 * (custom.py:1133-1194).  Here the envs form contiguous blocks: block t is envs [first_t, first_t + envs_per_track[t]) on tracks[t],
 * first_t = the sum of the counts before t.  Block t behaves bit for bit like a handle of ftgp_create with
 *     track = tracks[t], n_envs = envs_per_track[t], env_base = cfg->env_base + first_t
 * and everything else (vehicle, n_rays, fan, lidar_mode, map_size, dt, spawn mode, seed, ...) from *cfg.  cfg->track is ignored.
 * 1 <= n_tracks <= FTGP_MAX_TRACKS, every count >= 1, the counts sum to cfg->n_envs.  Every track gets the checks of ftgp_create (an
 * error names the track's index); all checks run before the device probe.  With one track the handle is ftgp_create's.
 * Every entry works on such a handle with its documented meaning over all envs, except ftgp_get_distance_field and ftgp_comm_init,
 * which return FTGP_ERR_STATE on a handle with more than one track (multi-rank runs of multi-track handles are not supported).
 */
#define FTGP_MAX_TRACKS 16
int ftgp_create_tracks(const FtgpConfig *cfg, const FtgpTrack *tracks, const int32_t *envs_per_track, int n_tracks, FtgpEnv **out);

/*
 * Reset.  Replaces Mujoco.reload() = mj_resetData + VehicleState rebuild + position_vehicles
 * (custom.py:1089-1128,1232-1245,81-87).  mask: NULL = all envs, else uint8[n_envs], non-zero = reset.
 * After reset: qvel = 0, ctrl = 0, LiDAR ranges = 0 (custom.py:1092), steps of the
 * env = 0, race state cleared, progress evaluated once at the spawn pose.
 */
int ftgp_reset(FtgpEnv *env, const uint8_t *mask);

/*
 * Controls.  Replaces data.ctrl[forward] = speed; data.ctrl[turn] = steering_angle
 * (custom.py:1421-1423; drive.py:82-83).  ctrl: double[n_envs*cars_per_env][2] = (speed, steering_angle).
 * car_mask (may be NULL): uint8 per car, 0 = leave that car's ctrl unchanged -- the reference's
 * behaviour when a driver raises (custom.py:1409-1411).
 */
int ftgp_set_ctrl(FtgpEnv *env, const double *ctrl, const uint8_t *car_mask);

/*
 * n_steps iterations of: sensors at the current pose -> integrate one dt -> steps += 1 ->
 * lap progress at the new pose.  Replaces mujoco.mj_step + steps += 1 (custom.py:1425-1426;
 * drive.py:89) followed by the progress block of the next loop iteration (custom.py:1340-1372).
 * Controls stay at their last ftgp_set_ctrl value.
 */
int ftgp_step(FtgpEnv *env, int n_steps);

/*
 * Same loop with the driver evaluated on the device between progress and integrate:
 * per step: policy(ranges of the previous step) -> ctrl -> sensors -> integrate -> progress.
 * This is the throughput path; one launch covers all n_steps.  The ranges a caller reads afterwards (ftgp_get_lidar and its kin) are
 * those of the launch's last step; the steps before it leave no ranges but the ones their drivers read (FTGP_SCAN_EVERY_STEP=1: all).
 */
int ftgp_rollout(FtgpEnv *env, int policy, int n_steps);

/*
 * The roster on the device: policies = int32[cars_per_env], the bundled driver (FTGP_POLICY_LOBOTOMY / NIDC / FAST / RANDOM) of
 * car slot k of every env; ftgp_rollout(FTGP_POLICY_PER_CAR, n) and ftgp_policy_eval(FTGP_POLICY_PER_CAR, ...) then evaluate each
 * car with its own driver.  Replaces the per-vehicle Driver() instances the reference builds from the roster's "driver" strings
 * and calls one by one (custom.py:1097-1104,1398-1411; template/cars/cars.json: nidc, fast, nidc).  Survives ftgp_reset.
 * FTGP_POLICY_NET0 .. NET3 (ftgp_set_net) are accepted too, here and in the roster of ftgp_device_io_config: a slot driven by a network.
 */
int ftgp_set_car_policies(FtgpEnv *env, const int32_t *policies);

/*
 * Device I/O: a vectorised environment stepped from device buffers, for drivers that live on the GPU (a learned driver, any batched
 * policy over the scan), with rewards, episode ends and auto-reset on the device.  The reference steps one world with one Python
 * driver call per car (custom.py:1398-1426); nothing there batches, so the rules below are this library's own, built from the
 * reference's pieces as cited.
 *
 * ftgp_device_io_config sets the slot table and the episode rules (it may synchronise; call it once, or between phases):
 *   roster             int32[cars_per_env] (host) or NULL (= every slot external).  FTGP_POLICY_HOST marks an external slot, driven by
 *                      the caller's actions; the other slots take FTGP_POLICY_LOBOTOMY / NIDC / FAST / RANDOM, the bundled drivers on the
 *                      device (template/cars/cars.json races nidc, fast, nidc).  At least one slot must be external.  This table is kept
 *                      apart from ftgp_set_car_policies' roster: ftgp_rollout(FTGP_POLICY_PER_CAR) and ftgp_policy_eval behave as if the
 *                      device path had never run.
 *   max_episode_steps  truncation: env steps since the env's last reset >= this; <= 0 = never
 *   action_repeat      physics steps per ftgp_step_device call, >= 1
 *   auto_reset         non-zero: envs that end in a call are reset at the end of that call
 * n_ext below = the number of external slots.
 */
typedef struct FtgpDeviceIoConfig {
    const int32_t *roster;
    int64_t max_episode_steps;
    int32_t action_repeat;
    int32_t auto_reset;
} FtgpDeviceIoConfig;
int ftgp_device_io_config(FtgpEnv *env, const FtgpDeviceIoConfig *cfg);

/*
 * One call of ftgp_step_device (it only enqueues work and never blocks the host):
 *   1. the handle's stream waits for `stream` (an event recorded there); at the end `stream` waits for the handle's stream;
 *   2. external car i of env e takes ctrl = ((double)action[e][i][0], (double)action[e][i][1]) -- (0, 0) once it has finished, the
 *      reference's null driver (custom.py:1441-1447); every car's absolute_completion (ftgp_get_progress column 3) is noted;
 *   3. action_repeat steps of ftgp_rollout(FTGP_POLICY_PER_CAR) with the device-io slot table: external slots keep their controls
 *      (a finished car gets (0, 0) at every step), the other slots run their bundled drivers;
 *   4. reward[e][i] = absolute_completion after - before (an integer, exact in float32); terminated[e] = every external car of e has
 *      finished (custom.py:1367-1370); truncated[e] = not terminated, max_episode_steps > 0 and the env's steps >= max_episode_steps;
 *      with auto_reset, an env that ended has its obs rows copied to final_obs (if given) and is reset exactly as ftgp_reset(mask)
 *      resets it (spawn, ranges 0, steps 0, progress at the spawn pose);
 *   5. obs[e][i] = the ranges of external car i of env e as ftgp_get_lidar lays them out -- all zeros for an env just reset
 *      (custom.py:1092).
 * Every buffer is device memory on the handle's device, laid out densely as below; a host pointer is FTGP_ERR_ARG before anything is
 * enqueued.  Before ftgp_device_io_config: FTGP_ERR_STATE.  ftgp_last_kernel_ms reports the step kernel of the call.
 */
typedef struct FtgpDeviceStep {
    void *stream;                 /* hipStream_t the buffers are ordered on (e.g. torch's current stream); NULL = the null stream */
    const float *action;          /* float32[n_envs][n_ext][2] = (speed, steering_angle), external slots in slot order */
    float *obs;                   /* float32[n_envs][n_ext][n_rays] */
    float *reward;                /* float32[n_envs][n_ext] */
    uint8_t *terminated;          /* uint8[n_envs] */
    uint8_t *truncated;           /* uint8[n_envs] */
    float *final_obs;             /* optional float32[n_envs][n_ext][n_rays]: rows of envs reset in this call get the pre-reset obs;
                                     other rows are left as they were */
} FtgpDeviceStep;
int ftgp_step_device(FtgpEnv *env, const FtgpDeviceStep *io);

/*
 * Signals of the device step: what a training loop otherwise computes with further kernels over the scans, or reads back through the
 * host.  The reference has none of this (one world, one Python driver call per car); the pieces are its own: the scan rows of
 * ftgp_get_lidar, the car record, and the off_track flag of the progress block (custom.py:1343-1345).
 *
 * The signals setter is valid after ftgp_device_io_config only (FTGP_ERR_STATE before it), and a later ftgp_device_io_config puts the
 * defaults {1, 0, 0, 0} back; a NULL argument sets the defaults too.  FTGP_ERR_ARG: a pool < 1 or not dividing n_rays; a max range or a
 * penalty that is negative, NaN or infinite.  n_beams below = n_rays / scan_pool.
 *
 * Pooled scan: beam b of external car i of env e covers rays [b * pool, (b + 1) * pool) of the car's ftgp_get_lidar row, in binary32.
 *   scan_max_range == 0   ranges < 0 (no hit) are left out, beam = the minimum of the others, -1 for a beam without any hit;
 *   scan_max_range M > 0  every range r counts as r < 0 ? M : min(r, M); beam = the minimum of those, times inv, where
 *                         inv = 1.0f / M is divided once on the host in binary32 (the kernel multiplies).
 * With signals set, obs and final_obs of FtgpDeviceStep are float32[n_envs][n_ext][n_beams].  An env reset in the call gets the beams
 * of its pre-reset rows in final_obs and zeros in obs; a finished car's beams are zeros (its scan is).
 *
 * reward[e][i] = (float)(absolute_completion after - before); if the car is off_track after the call's steps, reward - off_track_penalty
 * (one binary32 subtraction, in every call while the car stays off-track).  terminated[e] = every external car of e has finished, or
 * terminate_off_track is set and some external car of e is off_track.  truncated, auto_reset and final_obs: as ftgp_step_device.
 */
#define FTGP_STATE_FLOATS 8
typedef struct FtgpDeviceSignals {
    int32_t scan_pool;            /* >= 1 and a divisor of n_rays; 1 = one beam per ray */
    float   scan_max_range;       /* 0 = raw ranges; > 0 = clip and scale to [0, 1] */
    int32_t terminate_off_track;  /* non-zero: an env also terminates when an external car of it is off_track */
    float   off_track_penalty;    /* >= 0, subtracted from the reward of an external car that is off_track after the call */
} FtgpDeviceSignals;
int ftgp_device_io_signals(FtgpEnv *env, const FtgpDeviceSignals *signals);

/*
 * The device step with state rows: the same call (the one-argument form is this one with extra = NULL), plus, per external car,
 * float32[FTGP_STATE_FLOATS] taken from the car's record after the call's steps -- for an env reset in the call, after the reset,
 * from the spawn state; its pre-reset rows go to final_state, where only rows of envs reset in the call are written.  With
 * c = qw*qw - qz*qz and s = 2.0*(qw*qz) in binary64, every entry rounded once to binary32:
 *   0 v_long = vx*c + vy*s    1 v_lat = vy*c - vx*s    2 wz (yaw rate)    3 u_speed, 4 u_steer (the controls in force)
 *   5 sqrt(dist2), the distance to the nearest centre-line point (custom.py:1343)    6 (double)lap_completion / 100.0 (column 2 of
 *   ftgp_get_progress)    7 off_track, 0 or 1
 * state / final_state: float32[n_envs][n_ext][FTGP_STATE_FLOATS], device memory on the handle's device like the other buffers (a
 * host pointer is FTGP_ERR_ARG before anything is enqueued); either may be NULL.  With default signals and no state buffer the call
 * launches exactly the kernels of the one-argument form.
 */
typedef struct FtgpDeviceStepExtra {
    float *state;
    float *final_state;
} FtgpDeviceStepExtra;
int ftgp_step_device_ex(FtgpEnv *env, const FtgpDeviceStep *io, const FtgpDeviceStepExtra *extra);

/* The state rows of the current state, without a step (e.g. after ftgp_reset): float32[n_envs][n_ext][FTGP_STATE_FLOATS] in device
 * memory, ordered on `stream` like a device step (only enqueues).  After ftgp_device_io_config only (FTGP_ERR_STATE before it). */
int ftgp_state_device(FtgpEnv *env, void *stream, float *state);

/*
 * Contacts of the device step: did the car hit something.  The reference ends nothing on a contact (MuJoCo resolves it and the race
 * goes on, custom.py:1425); the pieces are this library's own contact geometry, the one K1's penalty forces use (DESIGN.md "K1").
 *
 * The contact row of a car, float32[FTGP_CONTACT_FLOATS], is evaluated at the car's pose as it stands: in a device step at the pose
 * after the call's steps, before any reset.  Everything is binary64 and every entry is rounded once to binary32.  With
 * ch = 1.0 - 2.0*(qz*qz) and sh = 2.0*(qw*qz):
 *   0 wall_pen    the deepest wall penetration over the car's wall circles.  The chassis circles k = 0..2 sit at body (contact_x[k], 0)
 *                 with radius contact_radius, world centre (x + ch*contact_x[k], y + sh*contact_x[k]); with bubble_wrap there are also
 *                 the four softeners at body (wheel_x[k], wheel_y[k]) with radius softener_radius, world centre
 *                 (x + (ch*wx - sh*wy), y + (sh*wx + ch*wy)).  A circle (centre (px, py), radius r) is looked up on the track's image:
 *                   u = (px - origin_x) * inv_px_x, w = (origin_y - py) * inv_px_y (inv_px = 1.0 / px_size, divided once), ix = floor(u),
 *                   iy = floor(w); a centre off the image (ix or iy outside [0, width) x [0, height)) touches nothing;
 *                   the wall pixels (cx, cy) of the rectangle |cx - ix| <= ceil(r * inv_px_x), |cy - iy| <= ceil(r * inv_px_y) on the image:
 *                   x0 = origin_x + (double)cx * px_size_x, x1 = x0 + px_size_x, y1 = origin_y - (double)cy * px_size_y, y0 = y1 - px_size_y,
 *                   (qx, qy) = (px, py) clamped to [x0, x1] x [y0, y1], ex = px - qx, ey = py - qy; the pixel touches when
 *                   ex*ex + ey*ey < r*r, and its penetration is r - sqrt(ex*ex + ey*ey).
 *                 The circle's penetration is the largest over its touching pixels -- exactly the `pen` K1's wall force starts from at that
 *                 pose.  0 when no circle touches.
 *   1 car_pen     the deepest overlap with an env-mate, over every mate b != a of the env that has not finished and the nine pairs (i, j)
 *                 of chassis circles: P = (x_a + ch_a*contact_x[i], y_a + sh_a*contact_x[i]), Q likewise of b with j, e = P - Q,
 *                 d2 = ex*ex + ey*ey; a pair counts when 0 < d2 < r2*r2, r2 = 2.0*contact_radius, with overlap r2 - sqrt(d2).  Cars of
 *                 bundled drivers are mates like any other.  0 when no pair counts.
 *   2 wall_count  the number of the car's wall circles that touch, 0 to 7
 *   3 car_count   the number of mates with at least one counting pair, 0 to 7
 * A finished car collides with nothing (custom.py:1452-1457): its row is all zeros and nobody counts it as a mate.  The test is
 * geometric overlap: a circle that penetrates but separates fast enough for K1's force to vanish (mag <= 0) still counts.  On a
 * multi-track handle the wall frame (bitmap, size, origin, pixel sizes) is the one of the env's track.
 *
 * The contacts setter is valid after ftgp_device_io_config only (FTGP_ERR_STATE before it); NULL turns contacts off, and so does a
 * later ftgp_device_io_config; ftgp_device_io_signals leaves them alone.  FTGP_ERR_ARG: a penalty that is negative, NaN or infinite.
 * A struct of all zeros still turns the contact rows on: it changes no reward and ends no episode.  With contacts on, a device step
 * evaluates every car's row once, between its steps and its episode rules:
 *   reward[e][i]   the value of ftgp_device_io_signals' rule (off_track_penalty subtracted as there), then - wall_penalty if the car's
 *                  wall_count > 0, then - car_penalty if its car_count > 0: binary32 subtractions in this order;
 *   terminated[e]  that rule's value, or terminate_on_wall and some external car of e has wall_count > 0, or terminate_on_car and some
 *                  external car of e has car_count > 0;
 *   truncated, auto_reset, final_obs: unchanged.
 * The rows are those of the pose after the call's steps: a contact that began and ended inside a call with action_repeat > 1 is not seen.
 */
#define FTGP_CONTACT_FLOATS 4
typedef struct FtgpDeviceContacts {
    int32_t terminate_on_wall;    /* non-zero: an env also terminates when an external car of it has wall_count > 0 */
    int32_t terminate_on_car;     /* ... car_count > 0 */
    float   wall_penalty;         /* >= 0, finite */
    float   car_penalty;          /* >= 0, finite */
} FtgpDeviceContacts;
int ftgp_device_io_contacts(FtgpEnv *env, const FtgpDeviceContacts *contacts);

/*
 * The device step with contact rows: ftgp_step_device_ex(e, io, x) is this call with contacts = NULL.  contact / final_contact:
 * float32[n_envs][n_ext][FTGP_CONTACT_FLOATS], device memory on the handle's device (a host pointer is FTGP_ERR_ARG before anything is
 * enqueued); either may be NULL.  An env reset in the call gets its pre-reset rows in final_contact (only such rows are written there)
 * and zeros in contact, like obs.  Contact buffers while contacts are off: FTGP_ERR_STATE.  With contacts off and no contact buffers
 * the call launches exactly the kernels of ftgp_step_device_ex.
 */
typedef struct FtgpDeviceStepContacts {
    float *contact;
    float *final_contact;
} FtgpDeviceStepContacts;
int ftgp_step_device_contacts(FtgpEnv *env, const FtgpDeviceStep *io, const FtgpDeviceStepExtra *extra, const FtgpDeviceStepContacts *contacts);

/* The external cars' contact rows at the current state, without a step: float32[n_envs][n_ext][FTGP_CONTACT_FLOATS] in device memory,
 * ordered on `stream` like ftgp_state_device (only enqueues).  After ftgp_device_io_config (FTGP_ERR_STATE before it); contacts need
 * not be on. */
int ftgp_contacts_device(FtgpEnv *env, void *stream, float *contact);

/*
 * Track frame of the device step: where the car is on the track, where the track points, and what lies ahead.  State entry 5 is an
 * unsigned distance to a centre-line POINT and the reward counts whole points; the row below projects the pose on the centre-line
 * itself.  The reference has none of this; the pieces are its centre-line (the 100 path points) and the nearest-point search of the
 * progress block (custom.py:1343).
 *
 * The frame row of a car, float32[FTGP_FRAME_FIXED + 2*n_ahead], is evaluated at the car's pose (x, y, qw, qz) as it stands, for a
 * finished car too (it is pure geometry).  All arithmetic is binary64 with one rounding per operation (no contraction; / and sqrt are
 * IEEE; no atan2, sin or cos).  P[i] = (X_i, Y_i) are the 100 centre-line points of the env's track; indices are taken mod 100, the
 * path is a closed loop.
 *   1. Nearest point.  c = the first index of the smallest d_i = dx*dx + dy*dy, dx = X_i - x, dy = Y_i - y (the progress block's
 *      expression and its first-minimum rule).  off = d_c > 1.0.
 *   2. Projection on segment a -> a+1.  ex = X_{a+1} - X_a, ey = Y_{a+1} - Y_a, L2 = ex*ex + ey*ey; rx = x - X_a, ry = y - Y_a.
 *      If L2 == 0 (a duplicated point): ex = 1, ey = 0, L2 = 1 and t = 0.  Otherwise t = (rx*ex + ry*ey) / L2, then t < 0 -> 0,
 *      t > 1 -> 1.  Foot point fx = X_a + t*ex, fy = Y_a + t*ey; gx = x - fx, gy = y - fy, g2 = gx*gx + gy*gy.
 *   3. Segment choice.  Step 2 for a = (c + 99) % 100 (segment A) and for a = c (segment B); A is taken only if g2_A < g2_B, otherwise
 *      B.  Below a, ex, ey, L2, rx, ry, t are those of the segment taken, and len = sqrt(L2).
 *   4. Heading of the car: ch = qw*qw - qz*qz, sh = 2.0*(qw*qz) (as in the state row).
 *   5. The fixed entries, each rounded once to binary32:
 *        0 lat    = (ex*ry - ey*rx) / len      signed lateral offset, positive = left of the direction of travel
 *        1 cos_h  = (ex*ch + ey*sh) / len
 *        2 sin_h  = (ey*ch - ex*sh) / len      entries 1 and 2: the track's tangent in the body frame; (1, 0) = aligned with the track,
 *                                              sin_h > 0 = the track turns away to the car's left
 *        3 s_norm = s / 100.0, s = (double)a + t, and s = s - 100.0 if s >= 100.0      the continuous lap position
 *   6. Look-ahead, k = 0 .. n_ahead - 1: q = (a + 1 + k*stride) % 100, dx = X_q - x, dy = Y_q - y;
 *        entry 4 + 2k = dx*ch + dy*sh (body-frame forward), entry 5 + 2k = dy*ch - dx*sh (body-frame left).
 * On a multi-track handle the path is the one of the env's track.
 *
 * The frame setter is valid after ftgp_device_io_config only (FTGP_ERR_STATE before it); NULL turns the frame off, and so does a
 * later ftgp_device_io_config; the signals and contacts setters leave the frame alone, and the frame leaves the spawn rule alone.
 * FTGP_ERR_ARG, before anything changes: n_ahead outside 0 .. FTGP_MAX_LOOKAHEAD, stride outside 1 .. 50, reserved != 0.  A struct
 * {0, 1, 0, 0} still turns the fixed entries on.
 *
 * Dense progress reward (dense_progress != 0).  For external car i of env e: (s0, off0) are s and off of the frame at the pose the
 * call begins with, (s1, off1) at the pose after the call's steps, before any reset (both s unrounded, binary64).  ds = s1 - s0;
 * if ds >= 50.0, ds = ds - 100.0; if ds < -50.0, ds = ds + 100.0; if off0 or off1, or the car had finished when the call began,
 * ds = 0.0 (the progress block freezes off the track, custom.py:1345; this also keeps a nearest-point jump across a fold of the track
 * out of the reward).  The base reward is (float)ds in the place of the integer difference; the off-track, wall and car penalties
 * follow as binary32 subtractions in the order given above.  With dense_progress == 0 the reward is unchanged to the bit.
 */
#define FTGP_FRAME_FIXED 4
#define FTGP_MAX_LOOKAHEAD 16
typedef struct FtgpDeviceFrame {
    int32_t n_ahead;              /* look-ahead points per row, 0 .. FTGP_MAX_LOOKAHEAD */
    int32_t stride;               /* path points between two of them, 1 .. 50 */
    int32_t dense_progress;       /* non-zero: the dense progress reward */
    int32_t reserved;             /* 0 */
} FtgpDeviceFrame;
int ftgp_device_io_frame(FtgpEnv *env, const FtgpDeviceFrame *frame);

/*
 * The device step with frame rows: ftgp_step_device_contacts(e, io, x, c) is this call with frame = NULL.  frame / final_frame:
 * float32[n_envs][n_ext][FTGP_FRAME_FIXED + 2*n_ahead], device memory on the handle's device (a host pointer is FTGP_ERR_ARG before
 * anything is enqueued); either may be NULL, and dense_progress works without them.  Rows are those of the pose after the call's
 * steps.  An env reset in the call gets its pre-reset rows in final_frame (only such rows are written there) and, in frame, the rows
 * evaluated again at the spawn pose -- like the state rows, not the contact rows: a look-ahead of zeros would be a lie.  Frame buffers
 * while the frame is off: FTGP_ERR_STATE.  With the frame off and no frame buffers the call launches exactly the kernels of
 * ftgp_step_device_contacts.
 */
typedef struct FtgpDeviceStepFrame {
    float *frame;
    float *final_frame;
} FtgpDeviceStepFrame;
int ftgp_step_device_frame(FtgpEnv *env, const FtgpDeviceStep *io, const FtgpDeviceStepExtra *extra, const FtgpDeviceStepContacts *contacts,
                           const FtgpDeviceStepFrame *frame);

/* The external cars' frame rows at the current state, without a step (e.g. after ftgp_reset), with the n_ahead and stride of the
 * frame setter: float32[n_envs][n_ext][FTGP_FRAME_FIXED + 2*n_ahead] in device memory, ordered on `stream` like ftgp_state_device
 * (only enqueues).  After ftgp_device_io_config (FTGP_ERR_STATE before it); with the frame off, n_ahead = 0 and the rows are the fixed
 * entries. */
int ftgp_frame_device(FtgpEnv *env, void *stream, float *frame);

/*
 * Rival rows of the device step: where the other cars of the env are, how fast they close, and whether the car is in front.  The scan
 * shows a mate only as a few short rays; the row below says it outright.  The reference has none of this; the pieces are the car
 * records, the nearest-point search of the frame row, absolute_completion and finish_step (the order of ftgp_get_winners).
 *
 * The rival row of car a, float32[FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS*n_rivals], is evaluated at the records as they stand.  The
 * arithmetic rules are those of the frame row: all arithmetic in binary64, one rounding per operation, no contraction, / and sqrt are
 * IEEE, every entry rounded once to binary32.  Cars are those of a's env, indexed by slot; the path is that of the env's track.
 *   1. Per car b: its place on the track.  Steps 1 - 3 of the frame row at b's pose give c_b, t_b, the unrounded wrapped s_b and
 *      off_b (for a finished car too).  f_b = s_b - (double)c_b; if f_b >= 50.0, f_b -= 100.0; if f_b < -50.0, f_b += 100.0; if
 *      off_b, f_b = 0.0.  Race progress g_b = (double)absolute_completion_b + f_b, absolute_completion_b being column 3 of
 *      ftgp_get_progress: g_b counts from the car's own start point, it is what decides who reaches lap_target first, and it is
 *      continuous where the nearest point steps on.
 *   2. Race order.  For b != a, b is ahead of a when one of these holds:
 *        both have finished and (finish_step_b, b) < (finish_step_a, a), compared lexicographically with the 64-bit finish_step
 *          (the order of ftgp_get_winners);
 *        b has finished and a has not;
 *        neither has finished, and g_b > g_a;
 *        neither has finished, g_b == g_a and b < a.
 *      Otherwise b is not ahead.  Comparisons with NaN are false.
 *   3. The fixed entries:
 *        0 place      = 1 + the number of cars ahead of a; for a finished car its ftgp_get_winners place
 *        1 n_racing   = the number of cars of the env that have not finished
 *        2 gap_ahead  = the smallest g_b - g_a over unfinished b ahead of a; 0 if there is none or a has finished
 *        3 gap_behind = the smallest g_a - g_b over unfinished b != a not ahead of a; 0 if there is none or a has finished
 *   4. Mates.  The mates of a are the unfinished cars b != a -- a finished car is a ghost (custom.py:1441-1466) -- and a finished a
 *      has no mates.  They are sorted by d2 = dx*dx + dy*dy, dx = x_b - x_a, dy = y_b - y_a, ascending, on equal d2 the smaller slot
 *      first; the first n_rivals of them fill the row's mate slots k = 0, 1, ...  With ch = qw*qw - qz*qz and sh = 2.0*(qw*qz) of a,
 *      chb and shb likewise of b, dvx = vx_b - vx_a and dvy = vy_b - vy_a, entry FTGP_RIVAL_FIXED + 8k + i is
 *        0 fwd       = dx*ch + dy*sh           the mate's position in a's body frame, forward
 *        1 left      = dy*ch - dx*sh           ... and left
 *        2 cos_rel   = chb*ch + shb*sh         the mate's heading in a's frame
 *        3 sin_rel   = shb*ch - chb*sh
 *        4 v_fwd     = dvx*ch + dvy*sh         the relative velocity in a's frame, forward
 *        5 v_left    = dvy*ch - dvx*sh         ... and left
 *        6 track_gap = s_b - s_a; if >= 50.0, - 100.0; if < -50.0, + 100.0      path points along the centre-line, positive = the
 *                                              mate is further along
 *        7 present   = 1.0                     the slot holds a mate
 *      A slot without a mate is eight zeros; n_rivals may exceed cars_per_env - 1, so one policy shape serves every roster.
 *
 * The rivals setter is valid after ftgp_device_io_config only (FTGP_ERR_STATE before it); NULL turns rivals off, and so does a later
 * ftgp_device_io_config; the signals, contacts and frame setters leave rivals alone, and rivals leave them and the spawn rule alone.
 * Rivals need no frame: they run their own search.  FTGP_ERR_ARG, before anything changes: n_rivals outside 0 .. FTGP_MAX_RIVALS,
 * place_weight negative, NaN or infinite, a reserved field != 0.  A struct {0, 0, 0, 0} still turns the fixed entries on.
 *
 * Place reward (place_weight w != 0).  p0 is a's place at the records the call begins with, p1 its place after the call's steps,
 * before any reset.  After the off-track, wall and car penalties, in their order: reward = reward + w * (float)(p0 - p1) -- one
 * binary32 multiplication and one binary32 addition, not fused; the term is 0 if the car had finished when the call began.  With
 * w == 0 the reward is unchanged to the bit.
 */
#define FTGP_RIVAL_FIXED 4
#define FTGP_RIVAL_FLOATS 8
#define FTGP_MAX_RIVALS 7
typedef struct FtgpDeviceRivals {
    int32_t n_rivals;             /* mate slots per row, 0 .. FTGP_MAX_RIVALS */
    int32_t reserved;             /* 0 */
    float place_weight;           /* w of the place reward, >= 0 and finite; 0 = none */
    float reserved_f;             /* 0 */
} FtgpDeviceRivals;
int ftgp_device_io_rivals(FtgpEnv *env, const FtgpDeviceRivals *rivals);

/*
 * The device step with rival rows: ftgp_step_device_frame(e, io, x, c, f) is this call with rivals = NULL.  rival / final_rival:
 * float32[n_envs][n_ext][FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS*n_rivals], device memory on the handle's device (a host pointer is
 * FTGP_ERR_ARG before anything is enqueued); either may be NULL, and the place reward works without them.  Rows are those of the
 * records after the call's steps.  An env reset in the call gets its pre-reset rows in final_rival (only such rows are written there)
 * and, in rival, the rows evaluated again at the spawn state, like the frame rows: everyone racing, velocities zero.  Rival buffers
 * while rivals are off: FTGP_ERR_STATE.  With rivals off and no rival buffers the call launches exactly the kernels of
 * ftgp_step_device_frame.
 */
typedef struct FtgpDeviceStepRivals {
    float *rival;
    float *final_rival;
} FtgpDeviceStepRivals;
int ftgp_step_device_rivals(FtgpEnv *env, const FtgpDeviceStep *io, const FtgpDeviceStepExtra *extra, const FtgpDeviceStepContacts *contacts,
                            const FtgpDeviceStepFrame *frame, const FtgpDeviceStepRivals *rivals);

/* The external cars' rival rows at the current state, without a step (e.g. after ftgp_reset), with the n_rivals of the rivals
 * setter: float32[n_envs][n_ext][FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS*n_rivals] in device memory, ordered on `stream` like
 * ftgp_frame_device (only enqueues).  After ftgp_device_io_config (FTGP_ERR_STATE before it); with rivals off, n_rivals = 0 and the
 * rows are the fixed entries. */
int ftgp_rivals_device(FtgpEnv *env, void *stream, float *rival);

/*
 * Spawn rule: random, wall-aware episode starts.  The reference places car i at path[(i+5)*2] in every episode (custom.py:1112,
 * 1232-1245); FtgpConfig.spawn_mode 0 / 1 are fixed poses too.  A rule is a property of the handle that every reset obeys once it is
 * set -- ftgp_reset with or without a mask and the auto-reset of the device step: start point, lateral offset, yaw and grid order are
 * drawn from the library's counter-based generator keyed by (seed, global env index, episode number), bounded by a per-track
 * wall-clearance table, and the progress offset is taken at the pose drawn.  With no rule set nothing changes, to the bit.
 *
 * Start table (host arithmetic at create, per track).  For path point p with spawn entry (X, Y, qw, qz): ch = 1.0 - 2.0*(qz*qz),
 * sh = 2.0*(qw*qz); the left normal is (-sh, ch), the right normal its negation.  delta = 0.5 * min(px_size_x, px_size_y),
 * K = (int)ceil(1.0 / delta) (1.0: the off-track distance, custom.py:1344).  On each side the samples k = 0 .. K sit at
 * (X + ((double)k*delta)*nx, Y + ((double)k*delta)*ny); a sample is blocked when its pixel -- found as the contact rows find theirs:
 * u = (px - origin_x)*inv_px_x, w = (origin_y - py)*inv_px_y, floor, bit (ix & 31) of word (ix >> 5) -- is a wall, or when it lies off
 * the image.  With m the first blocked k (K + 1 if none is), clear[p][side] = delta * (double)max(m - 1, 0).
 *
 * The draw, binary64 with one rounding per operation.  G = env_base + env, k = the env's episode counter, c = cars_per_env; splitmix64
 * and u01 are those of spawn_mode 1 and FTGP_POLICY_RANDOM; mul32(h, n) = ((h >> 32) * (uint64_t)n) >> 32.  start[] = the points
 * (first_point + i) % 100, i in [0, n_points), in this order, whose clear is >= margin on both sides; n_start their number.
 *   1. hE = splitmix64(splitmix64(seed ^ (0x5350574E52554C45 + (uint64_t)G)) ^ (uint64_t)k)
 *   2. b = start[mul32(hE, n_start)]
 *   3. slot[i] = i; with shuffle_grid: h = hE; for i = c-1 .. 1: h = splitmix64(h), j = mul32(h, i+1), swap slot[i] and slot[j]
 *   4. car a: p = (b + 2*slot[a]) % 100 (custom.py:1112's spacing); hC = splitmix64(hE ^ (0xD6E8FEB86659FD93 * (uint64_t)(a+1)));
 *      w = 2.0*u01(hC) - 1.0; v = 2.0*u01(splitmix64(hC)) - 1.0
 *   5. side = w >= 0 ? left : right; room = max(clear[p][side] - margin, 0.0); lat = (lateral_frac*w)*room;
 *      x = X_p + lat*(-sh), y = Y_p + lat*ch with ch, sh of the table's quaternion at p
 *   6. t = yaw_tan*v; n = sqrt(1.0 + t*t), cj = 1.0/n, sj = t/n; nw = qw*cj - qz*sj, nz = qz*cj + qw*sj; m = sqrt(nw*nw + nz*nz);
 *      qw' = nw/m, qz' = nz/m -- for t != 0; t == 0 (yaw_tan 0) leaves the table's (qw, qz) as they are, so that a rule without
 *      jitter on one point reproduces spawn_mode 0 to the bit (m is 1 only to within an ulp)
 *   7. offset = the first index of the smallest dx*dx + dy*dy over the 100 path points at (x, y), the progress block's arithmetic;
 *      the progress block then runs as at any reset: completion 0 and good_start 1 whatever the offset drawn.
 * Everything else of a reset is unchanged (velocities, controls and ranges 0, steps 0, lap times cleared).  A grid mate whose point is
 * blocked gets room 0: no lateral offset.  The rule promises no contact-free start; the contact row after the reset says.
 * With the rule on, every reset of env e spawns with k = episodes[e] and then sets episodes[e] = k + 1; with the rule off the counters
 * are not touched.  A shard [env_base, env_base + n) of a larger batch draws exactly what the same slice of the whole batch draws.
 *
 * ftgp_set_spawn_rule: NULL = off; valid on any handle; it may synchronise.  FTGP_ERR_ARG, before anything changes: first_point
 * outside 0..99, n_points outside 1..100, reserved != 0, a margin or yaw_tan that is negative, NaN or infinite, a lateral_frac
 * outside [0, 1], or a track without a start point left (the message names the track's index).  Every accepted call, NULL included,
 * zeroes the episode counters.  ftgp_device_io_config, ftgp_device_io_signals and ftgp_device_io_contacts leave the rule alone.
 */
typedef struct FtgpSpawnRule {
    int32_t first_point, n_points;  /* candidates (first_point + i) % 100, i in [0, n_points); 0..99 and 1..100 */
    int32_t shuffle_grid;           /* non-zero: the cars of an env draw their grid slots */
    int32_t reserved;               /* 0 */
    double  margin;                 /* >= 0, finite: a candidate with clear < margin on either side is no start point;
                                       lateral room on a side = max(clear - margin, 0) */
    double  lateral_frac;           /* in [0, 1]: share of that room the offset may use */
    double  yaw_tan;                /* >= 0, finite: tan of half the largest yaw offset */
} FtgpSpawnRule;
int ftgp_set_spawn_rule(FtgpEnv *env, const FtgpSpawnRule *rule);

/* int64[n_envs]: resets of every env since the rule was set (all zeros without a rule). */
int ftgp_get_episodes(FtgpEnv *env, int64_t *out);

/* double[FTGP_PATH_POINTS][6] of track `track` (0 .. n_tracks - 1): x, y, qw, qz of the spawn table, clear_left, clear_right; any handle,
 * with or without a rule.  FTGP_ERR_ARG for a track out of range. */
int ftgp_get_start_table(FtgpEnv *env, int track, double *out);

/* ---- Per-car vehicle dynamics (domain randomisation; no reference counterpart) -------------------------------------------------------
 * A handle may carry one dynamics row per car, FTGP_DYN_DOUBLES binary64 values, row of car (env * cars_per_env + car):
 *   0 mass  1 izz  2 friction  3 tire_damping  4 throttle_kv  5 throttle_force_limit  6 steer_kp  7 steer_damping
 * With the table on, car a integrates as a handle would whose FtgpConfig.vehicle is this handle's with these eight fields replaced
 * by row a.  Everything else stays the handle's: geometry, contact stiffness and damping, wheel and steering inertias, limits, kind,
 * the LiDAR.  The static wheel loads of car a follow from its mass by the rule of ftgp_create, in binary64, one rounding per
 * operation: wtot = mass * gravity; with a_f, a_r the distances of the front and rear axle from the origin,
 *   FTGP_VEHICLE_MUSHR     load fl = fr = 0.5 * (wtot * (a_r / (a_f + a_r))), bl = br = 0.5 * (wtot * (a_f / (a_f + a_r)))
 *   FTGP_VEHICLE_TRICYCLE  load l = r = 0.5 * (wtot * (a_f / (a_f + a_r))), caster = wtot * (a_r / (a_f + a_r))
 * so a row equal to the handle's own eight values reproduces the handle without a table to the bit.  FTGP_VEHICLE_TRICYCLE reads
 * entries 0-3 only; entries 4-7 are stored and ignored.
 *
 * The table is off on a new handle.  The first accepted setter call turns it on: every car's row starts as the handle's own values,
 * then the given rows of the masked envs replace theirs.  rows: [n_envs][cars_per_env][FTGP_DYN_DOUBLES]; env_mask: uint8[n_envs],
 * non-zero = take this env's rows, NULL = all envs (the mask of ftgp_reset).  ftgp_set_dynamics(env, NULL, NULL) turns the table off
 * and zeroes the rejected counter.  ftgp_reset, the auto-reset of a device step, ftgp_device_io_config, the ftgp_device_io_* setters
 * and ftgp_set_spawn_rule leave the table alone.  Valid on multi-track handles and on shards (rows are indexed by the handle's own
 * envs); FTGP_ERR_STATE on a FTGP_LIDAR_FAKELIDAR handle.
 *
 * A valid row has every entry finite, mass > 0, izz > 0 and entries 2-7 >= 0.  ftgp_set_dynamics (host buffers, synchronous) returns
 * FTGP_ERR_ARG before anything changes; the message names the first bad car and entry.  ftgp_set_dynamics_device (device buffers on
 * the handle's device) only enqueues (a handle's first setter call allocates the table and may synchronise), ordered on `stream` like ftgp_state_device: the handle's stream waits for `stream`, and
 * `stream` for the work.  FTGP_ERR_ARG for a buffer that is not device memory, before anything is enqueued.  It cannot look at the
 * values without a synchronisation: a car whose new row is invalid keeps its old row, and a device counter goes up by one.
 * ftgp_get_dynamics (host, synchronous): the rows in force, double[n_cars][FTGP_DYN_DOUBLES], and the number of rows rejected since
 * the table was turned on (either pointer may be NULL); with the table off, the handle's values for every car and 0. */
#define FTGP_DYN_DOUBLES 8
int ftgp_set_dynamics(FtgpEnv *env, const double *rows, const uint8_t *env_mask);
int ftgp_set_dynamics_device(FtgpEnv *env, void *stream, const double *rows, const uint8_t *env_mask);
int ftgp_get_dynamics(FtgpEnv *env, double *rows_out, int64_t *rejected_out);

/* ---- Env states on the device: save, restore, fork (no reference counterpart) ---------------------------------------------------------
 * Everything an env carries from one step to the next, as one record in device memory: the env's step count, its episode counter, its
 * cars' records (pose, velocities, the steering joint, the wheel spins, controls, fast.py's last steering angle, the race fields and
 * the lap-time ring), their dynamics records and their scans.  A save writes records, a load takes them back; a fork is a save
 * followed by a load with a row table.  Both only enqueue, like ftgp_set_dynamics_device.
 *
 * The record of one env is ftgp_env_state_bytes() bytes, a multiple of 16; every part starts on a 16-byte boundary.  With
 * c = cars_per_env and pad16(n) = (n + 15) & ~15, little-endian as the device stores it:
 *   offset  0  uint32 magic = 0x53454746 ("FGES")
 *           4  uint32 version = FTGP_ENV_STATE_VERSION
 *           8  int32  n_rays
 *          12  int32  cars_per_env
 *          16  int32  lidar_mode
 *          20  int32  reserved = 0
 *          24  uint64 track fingerprint (below) of the env's track
 *          32  int64  steps       (ftgp_get_steps)
 *          40  int64  episodes    (ftgp_get_episodes; 0 on a handle that never had a spawn rule)
 *          48  c car records of 448 bytes, car slot 0 first.  Doubles at byte 0, 8, ...: x, y, qw, qz, vx, vy, wz, qs, qsd (the steering
 *              joint's angle and rate), w[4] (wheel spins fl, fr, bl, br), u_speed, u_steer, last_steer, dist2 (ftgp_get_centre_dist2);
 *              int32 at byte 136: completion, laps, offset, n_times, good_start, finished, off_track, delta; int64 at byte 168: start,
 *              finish_step (meaningful while finished != 0); double times[FTGP_MAX_LAP_TIMES] at byte 192 (the ring of ftgp_get_lap_times)
 *          48 + 448 c  c dynamics records of FTGP_DYN_RECORD doubles: the car's FTGP_DYN_DOUBLES row, then its four static wheel loads.
 *              With the table off: the handle's own eight values and its wheel loads
 *          48 + 544 c  c scan rows of pad16(4 n_rays) bytes: the car's ftgp_get_lidar row as binary32 -- what the next driver call
 *              reads -- then zeros up to the boundary
 *   bytes_per_env = 48 + 544 c + c pad16(4 n_rays)          (4912 for 1 car x 1080 rays)
 *
 * Track fingerprint, computed once per track on the host at create, with splitmix64 the spawn rule's:
 *   h = 0; for every v of the sequence below, as uint64: h = splitmix64(h ^ v)
 *   sequence: width, height; the bitmap words [height][words_per_row] in row order, bits beyond the width cleared; the bit patterns of
 *   the 200 path doubles (x0, y0, x1, ...).
 *
 * ftgp_save_envs_device: env e of env_mask (uint8[n_envs] in device memory, non-zero = save; NULL = all envs: the mask of
 * ftgp_set_dynamics_device) writes row e of rows, n_rows rows of bytes_per_env bytes; n_rows >= n_envs (FTGP_ERR_ARG otherwise).  Rows
 * of other envs are not touched.
 *
 * ftgp_load_envs_device: env e takes row src_row[e] of rows (int32[n_envs] in device memory; NULL = row e, which needs
 * n_rows >= n_envs).  A negative entry leaves the env exactly as it is.  The kernel cannot report without a synchronisation: a row
 * whose index is >= n_rows, or whose magic, version, n_rays, cars_per_env, lidar_mode or fingerprint is not that of env e -- the
 * fingerprint of e's own track, so a row saved on another track of a multi-track handle is refused -- leaves the env untouched and
 * adds one to a device counter, which ftgp_get_env_state_rejected reads (host, synchronous).  The counter counts over the handle's
 * life: nothing resets it, no ftgp_device_io_config either; a caller compares two readings.  An env is loaded whole or not at all.
 * An accepted row writes steps; episodes, if the handle has or had a spawn rule (otherwise the entry is ignored); the car records;
 * the scans; and the dynamics records if the dynamics table is on.  With the table off they are ignored and the cars stay the
 * handle's vehicle.  The records are taken as they are: rows that a save wrote are valid, rows of other origin are the caller's.
 * The vehicle constants, dt, lap_target, seed, env_base and the device-io rules are neither in the record nor checked: loading across
 * handles that differ there is the caller's business.  Load touches neither the spawn rule, nor whether the dynamics table is on, nor
 * the device-io setters.  A row loaded into another env index continues bit for bit except for what is drawn per global env index:
 * FTGP_POLICY_RANDOM, the spawn rule's next draw and spawn_mode 1's pose at the next reset.
 *
 * Both are ordered on `stream` like ftgp_set_dynamics_device (the handle's stream waits for `stream`, and `stream` for the work) and are
 * valid on any handle after create: FTGP_LIDAR_FAKELIDAR, shards, multi-track handles and the tricycle included, with or without
 * ftgp_device_io_config.  A handle's first call allocates a few bytes and may synchronise.  FTGP_ERR_ARG, before anything is enqueued
 * and with the entry's name in front: a buffer that is not device memory on the handle's device or is smaller than the layout needs,
 * rows not 16-byte aligned, n_rows < n_envs where it is needed, n_rows < 1 or >= 2^31.  There is no env-to-env copy in place: save,
 * then load with src_row, which has no read-after-write hazard. */
#define FTGP_ENV_STATE_VERSION 1
#define FTGP_ENV_STATE_MAGIC 0x53454746u
#define FTGP_DYN_RECORD 12
int ftgp_env_state_bytes(FtgpEnv *env, size_t *bytes_per_env);
int ftgp_save_envs_device(FtgpEnv *env, void *stream, void *rows, int64_t n_rows, const uint8_t *env_mask);
int ftgp_load_envs_device(FtgpEnv *env, void *stream, const void *rows, int64_t n_rows, const int32_t *src_row);
int ftgp_get_env_state_rejected(FtgpEnv *env, int64_t *rejected);

/* The agents' observation rows at the state as it stands, without a step (e.g. after ftgp_load_envs_device, where obs is not zeros as
 * it is after a reset): float32[n_envs][n_ext][n_beams] in device memory, pooled, clipped and scaled by the signals in force, by the
 * device function the device step pools with -- a row equals to the bit what a step's obs holds for those scans.  Ordered on `stream`
 * like ftgp_state_device (only enqueues).  After ftgp_device_io_config only (FTGP_ERR_STATE before it). */
int ftgp_obs_device(FtgpEnv *env, void *stream, float *obs);

/* ---- Network drivers: a trained MLP as a device policy (no reference counterpart) ------------------------------------------------------
 * A handle carries up to FTGP_MAX_NETS networks, slots 0 .. 3.  Slot s is the device policy FTGP_POLICY_NET0 + s, usable wherever a
 * bundled driver is: ftgp_rollout, ftgp_set_car_policies, ftgp_policy_eval, the roster of ftgp_device_io_config.  Using a policy
 * whose slot is not defined is FTGP_ERR_STATE at the call that would launch it.  The driver is evaluated inside the step kernel's
 * driver phase, at every physics step, on the scan of the previous step -- what nidc and fast see.  It keeps no per-car state:
 * last_steer is untouched and the env-state record is what it was.
 *
 * Everything below is binary32 with one rounding per written operation unless it says binary64; fmaf(a, b, c) is the fused a*b + c
 * with one rounding; nothing else is contracted.  Comparisons with a NaN are false.
 *
 * Scan input.  s(r) = r < 0 ? M : (r < M ? r : M) for a range r of the car's ftgp_get_lidar row, M = max_range.  Beam b covers rays
 * [b*pool, (b+1)*pool): m = s(r_0); then for p = 1 .. pool-1 in this order, m = s(r_p) if s(r_p) < m; beam = m * inv with
 * inv = float32(1) / float32(M), divided once on the host.  For ranges without a NaN this is beam b of the device step's signals with
 * scan_pool = pool and scan_max_range = M.  Inputs 0 .. n_beams-1 are beams beam_first .. beam_first + n_beams - 1.
 * Restriction: the device drivers see only the scan window [eighth, n_rays - eighth), eighth = (int)(n_rays / 8.0) -- the samples
 * nidc and fast keep (nidc.py:18-19), 811 at 1080 rays -- so a network's beams must lie inside it: the rear quarter of the scan is
 * not an input.  At 1080 rays and pool 10 that allows beams 14 .. 93.
 *
 * State input (use_state = 1): inputs n_beams .. n_beams + 4 are entries 0 - 4 of the state row (v_long, v_lat, wz, u_speed,
 * u_steer), computed exactly as ftgp_state_device documents them -- binary64, each rounded once to binary32 -- from the car's record
 * at the moment the driver runs: the velocities after the previous step and the controls then in force.
 *
 * Layers.  n_layers in 1 .. FTGP_NET_MAX_LAYERS; n_in = n_beams + 5*use_state, 1 <= n_in <= FTGP_NET_MAX_INPUTS; width[l] is the number
 * of outputs of layer l: hidden widths 1 .. FTGP_NET_MAX_HIDDEN, width[n_layers - 1] exactly 2; entries of width[] past n_layers are 0.
 * Parameters: binary32 in torch's nn.Linear layout -- per layer W[n_out][n_in], then b[n_out] -- the layers one after the other in one
 * flat buffer.  Neuron j of a layer with input x: acc = b[j]; for k = 0 .. n_in-1 ascending, acc = fmaf(W[j][k], x[k], acc); output =
 * act(acc), hidden_act for every layer but the last, out_act for the last.
 *   FTGP_ACT_IDENTITY  acc
 *   FTGP_ACT_RELU      acc > 0 ? acc : 0
 *   FTGP_ACT_TANH      with clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v) (a NaN stays a NaN):
 *                      x = clamp(acc, -9, 9); x2 = x*x; d = 25; for k = 11, 10, .., 0: d = (float)(2k+1) + x2 / d; y = x / d;
 *                      output = clamp(y, -1, 1).  Lambert's continued fraction, twelve levels, evaluated from the inside out: within
 *                      2.7e-7 of tanh on [-12, 12]; before the last clamp it overshoots 1 by 2.4e-7.  / is IEEE division.
 *
 * Controls.  With (y0, y1) the outputs of the last layer: a = fmaf(y0, out_scale[0], out_offset[0]), b = fmaf(y1, out_scale[1],
 * out_offset[1]); u_speed = (double)a, u_steer = (double)b; if a or b is not finite, both are 0: a diverged network acts as the
 * null driver and cannot put a NaN into a car's state.  A finished car gets (0, 0) before the network is looked at (custom.py:1446).
 *
 * ftgp_set_net (host buffers; may synchronise) defines or replaces slot `slot`; desc = NULL clears it.  Everything is checked before
 * anything changes; FTGP_ERR_ARG names the field: a slot outside 0 .. 3; pool < 1 or not dividing n_rays; max_range not finite or
 * <= 0; n_beams < 1, beam_first < 0, beam_first*pool < eighth or (beam_first + n_beams)*pool > n_rays - eighth (the window rule);
 * use_state not 0 or 1; n_layers, n_in or a width out of range, the last width != 2; an unknown activation; out_scale / out_offset
 * not finite; reserved != 0; params = NULL.  FTGP_ERR_STATE on a FTGP_LIDAR_FAKELIDAR handle, as ftgp_set_dynamics.
 * ftgp_set_net_device replaces the parameters of a slot that is defined, from device memory on the handle's device in the same
 * layout; it only enqueues, ordered on `stream` like ftgp_set_dynamics_device (the handle's stream waits for `stream`, and `stream`
 * for the work) -- the self-play loop that refreshes a frozen opponent from the training network without leaving the device.  A host
 * pointer or a buffer too small is FTGP_ERR_ARG before anything is enqueued; a slot not defined is FTGP_ERR_STATE.
 * ftgp_get_net (host, synchronous): the description and the parameters in force, in the caller's layout, ftgp_net_param_count floats
 * = the sum over the layers of n_out*n_in + n_out; either pointer may be NULL; FTGP_ERR_STATE for a slot not defined.
 * ftgp_reset, the auto-reset of a device step, ftgp_device_io_config and the ftgp_device_io_* setters, ftgp_set_spawn_rule,
 * ftgp_set_dynamics and the env-state calls leave the networks alone.  Launches that name no network run exactly the kernels they
 * ran before any network was set. */
#define FTGP_POLICY_NET0      6  /* the network of slot 0 (ftgp_set_net) ... */
#define FTGP_POLICY_NET1      7
#define FTGP_POLICY_NET2      8
#define FTGP_POLICY_NET3      9  /* ... of slot 3 */
#define FTGP_MAX_NETS 4
#define FTGP_NET_MAX_LAYERS 4
#define FTGP_NET_MAX_INPUTS 256
#define FTGP_NET_MAX_HIDDEN 128
#define FTGP_NET_STATE_INPUTS 5
#define FTGP_ACT_IDENTITY 0
#define FTGP_ACT_RELU     1
#define FTGP_ACT_TANH     2
typedef struct FtgpNetDesc {
    int32_t pool;                 /* rays per beam, >= 1 and a divisor of n_rays */
    float   max_range;            /* M > 0, finite */
    int32_t beam_first, n_beams;  /* the beams taken, inside the drivers' scan window */
    int32_t use_state;            /* 0 or 1: five state inputs behind the beams */
    int32_t n_layers;             /* 1 .. FTGP_NET_MAX_LAYERS */
    int32_t width[FTGP_NET_MAX_LAYERS];   /* outputs per layer; width[n_layers - 1] = 2, the rest 0 */
    int32_t hidden_act, out_act;  /* FTGP_ACT_* */
    float   out_scale[2], out_offset[2];  /* the output map, finite */
    int32_t reserved;             /* 0 */
} FtgpNetDesc;
int ftgp_set_net(FtgpEnv *env, int slot, const FtgpNetDesc *desc, const float *params);
int ftgp_set_net_device(FtgpEnv *env, void *stream, int slot, const float *params);
int ftgp_get_net(FtgpEnv *env, int slot, FtgpNetDesc *desc_out, float *params_out);

/* Frame inputs: the track frame behind the beams and the state inputs, so that a policy trained on the device step's frame row
 * (ftgp_device_io_frame) can be a roster slot, be evaluated in one launch and be collected (ftgp_collect_device).
 * ftgp_set_net_frame is ftgp_set_net with one more struct; frame == NULL or enabled == 0 is ftgp_set_net to the letter, and
 * ftgp_set_net keeps defining a slot without frame inputs.
 *
 * Input width.  n_in = n_beams + 5*use_state + enabled*(FTGP_FRAME_FIXED + 2*n_ahead), 1 <= n_in <= FTGP_NET_MAX_INPUTS.  The frame
 * entries come last: inputs n_in - (FTGP_FRAME_FIXED + 2*n_ahead) .. n_in - 1 are entries 0, 1, .. of the frame row.
 * Frame entries.  The frame row of "Track frame" above, steps 1 - 6 verbatim, with the SLOT's n_ahead and stride: binary64 with one
 * rounding per operation, each entry rounded once to binary32, the first-minimum rule for c, segment B on a tie.  It is evaluated at
 * the car's record (x, y, qw, qz) at the moment the driver runs -- where the state inputs are taken -- and on a multi-track handle
 * with the path of the env's track.  The slot's frame inputs do not depend on ftgp_device_io_frame being on, nor on its n_ahead and
 * stride; they equal the device step's `frame` row of the same record when the two settings agree.  So what a net slot sees is what
 * an agent is given: cat(obs[beam_first .. beam_first + n_beams), state[0 .. 5), frame) of an agent whose env has scan_pool = pool,
 * scan_max_range = max_range and the same (n_ahead, stride).  (Rival rows as inputs: ftgp_set_net_rivals, below.)
 * A finished car still gets (0, 0) before the network is looked at.  ftgp_collect_device's x, inputs and next_inputs are this wider
 * vector, for a finished car too.  ftgp_get_net returns the parameters with the slot's true n_in (the first layer has n_in columns),
 * and ftgp_set_net_device takes them so: the same layout, a larger count.  The env-state record and the parameter block's layout are
 * what they were.
 *
 * The setter carries all of ftgp_set_net's checks and, before anything changes (a refused call leaves a defined slot in force),
 * FTGP_ERR_ARG naming the field for: enabled not 0 or 1; n_ahead outside 0 .. FTGP_MAX_LOOKAHEAD or stride outside 1 .. 50 -- checked
 * with enabled == 0 too, as ftgp_device_io_frame checks its struct --; reserved != 0; n_in > FTGP_NET_MAX_INPUTS.
 * ftgp_get_net_frame (host): the frame inputs of a defined slot as the setter was given them; a slot defined without frame inputs
 * reads {0, 0, 0, 0}.  FTGP_ERR_STATE for a slot not defined. */
typedef struct FtgpNetFrame {     /* 16 bytes */
    int32_t enabled;              /* 0 or 1: the frame row behind the beams and the state inputs */
    int32_t n_ahead;              /* look-ahead points, 0 .. FTGP_MAX_LOOKAHEAD */
    int32_t stride;               /* path points between two of them, 1 .. 50 */
    int32_t reserved;             /* 0 */
} FtgpNetFrame;
int ftgp_set_net_frame(FtgpEnv *env, int slot, const FtgpNetDesc *desc, const FtgpNetFrame *frame, const float *params);
int ftgp_get_net_frame(FtgpEnv *env, int slot, FtgpNetFrame *frame_out);

/* Rival inputs: the rival row behind the beams, the state inputs and the frame inputs, so that a racing policy trained on the device
 * step's rival row (ftgp_device_io_rivals) can be its own frozen opponent, be evaluated in one launch and be collected.
 * ftgp_set_net_rivals is ftgp_set_net_frame with one more struct; rivals == NULL or enabled == 0 is ftgp_set_net_frame to the letter,
 * and ftgp_set_net and ftgp_set_net_frame keep defining slots without rival inputs.
 *
 * Input width.  n_in = n_beams + 5*use_state + frame.enabled*(FTGP_FRAME_FIXED + 2*n_ahead) + enabled*(FTGP_RIVAL_FIXED +
 * FTGP_RIVAL_FLOATS*n_rivals), 1 <= n_in <= FTGP_NET_MAX_INPUTS.  The rival entries come last: inputs n_in - (FTGP_RIVAL_FIXED +
 * FTGP_RIVAL_FLOATS*n_rivals) .. n_in - 1 are entries 0, 1, .. of the rival row.
 * Rival entries.  The rival row of "Rival rows of the device step" above, steps 1 - 4 verbatim, with the SLOT's n_rivals: binary64 with
 * one rounding per operation and no contraction, each entry rounded once to binary32; the (d2, slot) order of the mates, the ghost
 * rule for finished cars and eight zeros for a slot without a mate; f_b = 0 for an off-track car and the 64-bit finish_step order
 * among finishers.  The row is evaluated on the records of ALL cars of the car's env at the moment the driver runs -- where the state
 * and frame inputs are taken; inside a launch of several steps, the records after the previous step -- and every car of the env
 * counts, whoever drives it.  On a multi-track handle the path is that of the env's track, for every mate's search.  The slot's rival
 * inputs do not depend on ftgp_device_io_rivals being on, nor on its n_rivals; they equal the device step's `rival` row of the same
 * records when the two n_rivals agree.  So what a net slot sees is cat(obs[beams], state[0 .. 5), frame, rival) of an agent.  With one
 * car per env the block is (1, 1, 0, 0, zeros): one policy shape serves every roster.
 * A finished car still gets (0, 0) before the network is looked at.  ftgp_collect_device's x, inputs and next_inputs are this wider
 * vector, for a finished car too: its place is its ftgp_get_winners place, its gaps are 0 and it has no mates.  ftgp_get_net and
 * ftgp_set_net_device use the slot's true n_in.  FtgpNetDesc, FtgpNetFrame, FtgpConfig, the env-state record and the parameter block's
 * layout are what they were.
 *
 * The setter carries all of ftgp_set_net_frame's checks and, before anything changes (a refused call leaves a defined slot in force),
 * FTGP_ERR_ARG naming the field for: enabled not 0 or 1; n_rivals outside 0 .. FTGP_MAX_RIVALS -- checked with enabled == 0 too --; a
 * reserved word != 0; n_in > FTGP_NET_MAX_INPUTS.
 * ftgp_get_net_rivals (host): the rival inputs of a defined slot as the setter was given them; a slot defined without rival inputs
 * reads {0, 0, {0, 0}}.  FTGP_ERR_STATE for a slot not defined. */
typedef struct FtgpNetRivals {    /* 16 bytes */
    int32_t enabled;              /* 0 or 1: the rival row behind the beams, the state inputs and the frame inputs */
    int32_t n_rivals;             /* mate slots, 0 .. FTGP_MAX_RIVALS */
    int32_t reserved[2];          /* 0 */
} FtgpNetRivals;
int ftgp_set_net_rivals(FtgpEnv *env, int slot, const FtgpNetDesc *desc, const FtgpNetFrame *frame,
                        const FtgpNetRivals *rivals, const float *params);
int ftgp_get_net_rivals(FtgpEnv *env, int slot, FtgpNetRivals *rivals_out);

/* ---- Network populations: one parameter set per env in a single launch (no reference counterpart) ------------------------------------
 * A defined slot may carry a population: n_members parameter sets of the slot's shape and an env-to-member map.  A car of env e (the
 * handle's local env index) driven by that slot is evaluated with the parameters of member env_member[e] -- in the step kernel's driver
 * phase (ftgp_rollout, ftgp_step_device and their kin), in ftgp_policy_eval and in ftgp_collect_device (Act and next_inputs).  Nothing
 * else about the network driver changes: the inputs, the order of operations, TANH, the guard and the finished-car rule are the text of
 * "Network drivers" above, with "the slot's parameters" read as "the parameters of the env's member".  Evolution strategies,
 * population-based training, a league of checkpoints, a sweep of policies: M sets side by side, no launch per set.
 *
 * ftgp_set_net_population (host buffers; may synchronise).  params = float32[n_members][count], count = the floats ftgp_get_net returns
 * for the slot (ftgp_set_net's layout with the slot's true n_in), member after member.  env_member = int32[n_envs], or NULL for
 * env_member[e] = e % n_members.  Everything is checked before anything changes, and a refused call leaves the slot as it was:
 * FTGP_ERR_STATE for a slot that is not defined; FTGP_ERR_ARG, naming the field, for a slot outside 0 .. 3, n_members outside
 * 0 .. n_envs, params == NULL with n_members > 0, an env_member entry outside [0, n_members).  A failed allocation is FTGP_ERR_HIP with
 * nothing changed.  n_members == 0 removes the population: the slot's single parameter set, which is kept throughout, is in force
 * again.  A second call replaces the population, members and map.
 *
 * ftgp_set_net_population_device replaces the members' parameters and/or the map of a slot that carries a population, from device
 * memory on the handle's device in the same layouts (NULL = keep), ordered on `stream` exactly as ftgp_set_net_device; it only
 * enqueues.  n_members stays what the host setter made it.  The buffers are checked as ftgp_step_device checks its own before anything
 * is enqueued; FTGP_ERR_STATE for a slot that is not defined or carries no population.  The map's entries cannot be checked without a
 * synchronisation: an entry outside [0, n_members) is taken as member 0.
 *
 * ftgp_get_net_population (host, synchronous): n_members (0 = no population); the map in force; the parameters of member `member` in
 * the caller's layout.  Each output may be NULL; asking for the map or for parameters of a slot without a population is FTGP_ERR_STATE,
 * a member outside [0, n_members) with params_out set is FTGP_ERR_ARG.
 *
 * With the other entries: ftgp_set_net, ftgp_set_net_frame and ftgp_set_net_rivals (re)define a slot without a population.
 * A call that gives a slot a population ends the slot's trainer (ftgp_train_begin).
 * ftgp_set_net_device on a slot with a population is FTGP_ERR_STATE (use ftgp_set_net_population_device).  ftgp_get_net keeps returning
 * the description and the slot's single set.  ftgp_reset, auto-reset, the spawn rule, the dynamics table and the ftgp_device_io_*
 * setters leave the population and the map alone, and so do the env-state calls: an env that loads another env's state keeps its own
 * member -- the member belongs to the env index, not to the state record, which is unchanged (FTGP_ENV_STATE_VERSION too).
 * Memory: a member takes the slot's library layout (every layer's outputs padded to 64) rounded up to 64 floats; with n_members different
 * members in flight every car streams its own weights, which the cars of one member share through L2. */
int ftgp_set_net_population(FtgpEnv *env, int slot, int n_members, const float *params, const int32_t *env_member);
int ftgp_set_net_population_device(FtgpEnv *env, void *stream, int slot, const float *params, const int32_t *env_member);
int ftgp_get_net_population(FtgpEnv *env, int slot, int32_t *n_members_out, int32_t *env_member_out, int member, float *params_out);

/* ---- Collected rollouts: T decisions of a network on the device, written down (no reference counterpart) ------------------------------
 * ftgp_collect_device drives every external slot of a device-io handle with network slot `slot` for n_decisions = T decisions, with
 * optional exploration noise, and records per decision what the network saw, what it proposed, what was applied and what came back.
 * One decision is one ftgp_step_device call's worth of work.  The call only enqueues.
 *
 * Everything in step 1 is binary32 with one rounding per written operation; fmaf(a, b, c) is the fused a*b + c with one rounding;
 * nothing else is contracted.  Comparisons with a NaN are false.  Decision t = 0 .. T-1:
 *   1. Act.  For external car i of env e, at the records and scans as they stand: x = the network's input vector exactly as "Scan
 *      input" and "State input" of ftgp_set_net define it -- the beams from the car's ftgp_get_lidar row, the state entries 0 - 4 from
 *      the car's record with the controls then in force, and, for a slot with frame inputs (ftgp_set_net_frame), the frame row of that
 *      record behind them, and, for a slot with rival inputs (ftgp_set_net_rivals), the rival row of the env's records behind those.  inputs[t][e][i] = x, for a finished car too.  A finished car gets mean =
 *      action = (0, 0) and the network is not looked at (the network driver's rule).  Otherwise, with y = the layers on x and k = 0, 1:
 *        m_k = fmaf(y_k, out_scale[k], out_offset[k])
 *        a_k = fmaf(std[k], noise[t][e][i][k], m_k)              (noise = NULL: every draw is 0; 0 * infinity is a NaN)
 *        a_k = a_k < lo[k] ? lo[k] : (a_k > hi[k] ? hi[k] : a_k)  (a NaN stays a NaN; an infinite a_k becomes the bound)
 *        if a_0 or a_1 is not finite, both are 0
 *      mean[t][e][i] = (m_0, m_1) as computed -- not guarded, so a diverged network shows -- and action[t][e][i] = (a_0, a_1).
 *   2. Step.  Steps 2 - 5 of ftgp_step_device run with action = action[t], under every rule in force: signals, contacts, frame, rivals
 *      and their rewards and terminations, max_episode_steps, action_repeat, auto_reset and the spawn rule.  reward[t], terminated[t]
 *      and truncated[t] are that call's outputs.  The obs and row buffers of the device step are not part of the record: they go to
 *      scratch memory of the handle's.
 *   3. Next inputs.  If next_inputs is given, next_inputs[t][e][i] = step 1's x at the state after the call's physics steps and before
 *      the reset of an env that ended (the reset is the finish kernel's) -- what a value bootstrap needs at a truncation.
 *   4. Dynamics on reset.  If reset_dynamics is given, the envs with terminated[t] | truncated[t] take rows [t], exactly as
 *      ftgp_set_dynamics_device with that mask would do it: an invalid row keeps the old one and counts as rejected, and the first
 *      decision turns the table on.  FTGP_ERR_STATE if auto_reset is off, and on a handle where ftgp_set_dynamics is.
 * The contract: after the call, the handle and the outputs are to the bit what T calls of ftgp_step_device_rivals fed action[0 .. T-1]
 * would leave -- with reset_dynamics, the masked ftgp_set_dynamics_device calls between them.  So the network is evaluated once per
 * decision and the action holds for action_repeat physics steps (a roster network is evaluated at every physics step); with
 * action_repeat = 1, noise = NULL, a clip that does not bind and no episode end, a collected agent moves bit for bit like a car of
 * ftgp_rollout(env, FTGP_POLICY_NET0 + slot, T).
 *
 * Ordering: the handle's stream waits for `stream` once at the start, and `stream` for the handle's once at the end; nothing blocks
 * the host.  A handle's first call allocates scratch memory and may synchronise.  Every buffer is device memory on the handle's
 * device, dense, at T times the size of one decision (computed in size_t).  Errors, all before anything is enqueued: FTGP_ERR_STATE
 * before ftgp_device_io_config or for a slot not defined (the roster's network slots included); FTGP_ERR_ARG, naming the field, for
 * n_decisions < 1, a slot outside 0 .. 3, std negative or not finite, lo or hi not finite or lo > hi, reserved != 0, a buffer that is
 * NULL (noise, next_inputs and reset_dynamics may be), not device memory on the handle's device or too small, and for a slot whose
 * beams cover more than 4048 rays (n_beams * pool; four cars' rays share a workgroup's 64 KiB of LDS). */
typedef struct FtgpCollect {
    void *stream;                 /* as FtgpDeviceStep.stream */
    int32_t slot;                 /* 0 .. FTGP_MAX_NETS-1, must be defined */
    int32_t n_decisions;          /* T >= 1 */
    float std[2];                 /* >= 0, finite */
    float lo[2], hi[2];           /* finite, lo[k] <= hi[k]: the action's clip */
    const float *noise;           /* optional float32[T][n_envs][n_ext][2], the caller's draws (e.g. one torch.randn); NULL = zeros */
    float *inputs;                /* float32[T][n_envs][n_ext][n_in] */
    float *mean;                  /* float32[T][n_envs][n_ext][2] */
    float *action;                /* float32[T][n_envs][n_ext][2] */
    float *reward;                /* float32[T][n_envs][n_ext] */
    uint8_t *terminated, *truncated;   /* uint8[T][n_envs] */
    float *next_inputs;           /* optional, as inputs: the state after decision t's steps, BEFORE any reset */
    const double *reset_dynamics; /* optional double[T][n_envs][cars_per_env][FTGP_DYN_DOUBLES] */
    int32_t reserved;             /* 0 */
} FtgpCollect;
int ftgp_collect_device(FtgpEnv *env, const FtgpCollect *c);

/* ---- Collected rollouts with values: a value net per slot, bootstrap values and advantages (no reference counterpart) ------------------
 * What an actor-critic learner needs next to a collected rollout, without a pass through the caller's framework: the critic's value at
 * every decision, its value at the state the decision led to (before any reset: the bootstrap of a truncation), and the advantages
 * and returns of generalised advantage estimation.
 *
 * Everything here is binary32 with one rounding per written operation; fmaf is the fused multiply-add with one rounding; nothing else is
 * contracted.  Comparisons with a NaN are false.
 *
 * The value net of slot s.  A defined network slot may carry one value net.  It reads the slot's own input vector x -- beams, state,
 * frame and rival entries exactly as the slot defines them, at the slot's true n_in -- and its layers are the "Layers" text of "Network
 * drivers" verbatim: acc = b[j], then one fmaf per k ascending, the same three activations and the same TANH; hidden widths
 * 1 .. FTGP_NET_MAX_HIDDEN, the last width exactly 1.  With y the single output of the last layer,
 *     v = fmaf(y, out_scale, out_offset)
 * and there is no guard: a diverged critic shows as a NaN or an infinity in the record.  Parameters: torch's nn.Linear layout in one
 * flat buffer, as ftgp_set_net takes them (the first layer has n_in columns); the count is the sum over the layers of n_out*n_in + n_out.
 * A value net has ONE parameter set: on a slot with a population (ftgp_set_net_population) every env uses that one set, whatever its
 * member; per-member critics are not provided.
 * The value net is evaluated by ftgp_collect_values_device alone -- never by the step kernel, ftgp_rollout or ftgp_policy_eval --, and
 * launches that name no value net run the kernels they ran before there was one, with the arguments they got.
 *
 * ftgp_set_value_net (host buffers; may synchronise) gives defined slot `slot` a value net or replaces it; desc = NULL clears it.
 * Everything is checked before anything changes and a refused call leaves the slot as it was.  FTGP_ERR_ARG names the field: a slot
 * outside 0 .. 3; n_layers outside 1 .. FTGP_NET_MAX_LAYERS; a hidden width outside 1 .. FTGP_NET_MAX_HIDDEN, the last width != 1, a
 * width behind the last layer != 0; an unknown activation; out_scale or out_offset not finite; reserved != 0; params = NULL.
 * FTGP_ERR_STATE for a slot that is not defined.
 * ftgp_set_value_net_device replaces the parameters of a value net that is there, from device memory on the handle's device in the
 * same layout; it only enqueues and never synchronises, ordered on `stream` exactly as ftgp_set_net_device (the handle's stream waits
 * for `stream`, and `stream` for the work): a critic changes at every iteration of its learner.  A host pointer or a buffer too small
 * is FTGP_ERR_ARG before anything is enqueued; a slot without a value net is FTGP_ERR_STATE.
 * ftgp_get_value_net (host, synchronous) mirrors ftgp_get_net: the description and the parameters in force, in the caller's layout;
 * either pointer may be NULL; FTGP_ERR_STATE for a slot without a value net.
 * With the other entries: ftgp_set_net, ftgp_set_net_frame and ftgp_set_net_rivals on a slot clear its value net (the input width may
 * change) and end its trainer (ftgp_train_begin), as ftgp_set_value_net itself does.  ftgp_set_net_device, ftgp_set_net_population and its device form, ftgp_reset, auto-reset, the spawn rule, the dynamics
 * table, the ftgp_device_io_* setters and the env-state calls leave it alone. */
typedef struct FtgpValueDesc {
    int32_t n_layers;                       /* 1 .. FTGP_NET_MAX_LAYERS */
    int32_t width[FTGP_NET_MAX_LAYERS];     /* hidden 1 .. FTGP_NET_MAX_HIDDEN, width[n_layers - 1] exactly 1, the rest 0 */
    int32_t hidden_act, out_act;            /* FTGP_ACT_* */
    float   out_scale, out_offset;          /* finite */
    int32_t reserved;                       /* 0 */
} FtgpValueDesc;
int ftgp_set_value_net(FtgpEnv *env, int slot, const FtgpValueDesc *desc, const float *params);
int ftgp_set_value_net_device(FtgpEnv *env, void *stream, int slot, const float *params);
int ftgp_get_value_net(FtgpEnv *env, int slot, FtgpValueDesc *desc_out, float *params_out);

/* ftgp_collect_values_device: ftgp_collect_device with the slot's value net evaluated along the way.  v == NULL is ftgp_collect_device
 * to the letter.  Otherwise everything ftgp_collect_device documents holds unchanged -- every buffer of c and the handle afterwards are
 * to the bit what ftgp_collect_device with the same c leaves -- and in addition, for decision t:
 *   1'. value[t][e][i] = the slot's value net on step 1's x, for every external car, finished or not: a finished car's policy is not
 *       looked at, its value is.
 *   3'. next_value[t][e][i] = the value net on step 3's x -- the state after the decision's physics steps and before any reset --
 *       whether or not c->next_inputs is given: the bootstrap of a truncation needs no next_inputs.
 *   5.  If advantage is given, the advantage scan below runs after decision T-1 over the call's own reward, value, next_value,
 *       terminated and truncated, and writes advantage and ret.
 * Ordering and buffers as ftgp_collect_device.  Errors, all before anything is enqueued: those of ftgp_collect_device for c;
 * FTGP_ERR_STATE for a slot without a value net; FTGP_ERR_ARG, naming the field, for gamma or lam not finite or outside [0, 1], for
 * reserved != 0, for one of advantage and ret given without the other, and for a buffer that is NULL (the optional pair may be), not
 * device memory on the handle's device or too small.
 *
 * The advantage scan (ftgp_gae_device, and step 5 above).  Rows are the n_envs * n_ext external cars of a device-io handle; reward,
 * value, next_value, advantage and ret are float32[T][n_envs][n_ext], terminated and truncated uint8[T][n_envs], T = n_decisions.
 * gl = gamma * lam, rounded once on the host.  For each row, for t = T-1 down to 0, with term and trunc the bytes of the row's env at t:
 *     nv = term ? 0.0f : next_value[t]
 *     d  = fmaf(gamma, nv, reward[t]) - value[t]
 *     A  = (t == T-1 || term || trunc) ? d : fmaf(gl, A_next, d)
 *     advantage[t] = A;  ret[t] = A + value[t];  A_next = A
 * Non-finite values pass through as the arithmetic gives them.  ftgp_gae_device only enqueues, ordered on `stream` like
 * ftgp_state_device: a learner that rescales or reshapes rewards after collection recomputes its advantages with it.  FTGP_ERR_STATE
 * before ftgp_device_io_config; FTGP_ERR_ARG, naming the field, for n_decisions < 1, gamma or lam not finite or outside [0, 1], and a
 * buffer that is NULL, not device memory on the handle's device or too small. */
typedef struct FtgpCollectValues {
    float gamma, lam;            /* finite, in [0, 1] */
    float *value;                /* float32[T][n_envs][n_ext] */
    float *next_value;           /* float32[T][n_envs][n_ext] */
    float *advantage, *ret;      /* optional, both or neither: float32[T][n_envs][n_ext] */
    int32_t reserved[2];         /* 0 */
} FtgpCollectValues;
int ftgp_collect_values_device(FtgpEnv *env, const FtgpCollect *c, const FtgpCollectValues *v);
int ftgp_gae_device(FtgpEnv *env, void *stream, int n_decisions, float gamma, float lam,
                    const float *reward, const float *value, const float *next_value,
                    const uint8_t *terminated, const uint8_t *truncated, float *advantage, float *ret);

/* ---- Training on the device: PPO gradients of a slot's two nets and an Adam step (no reference counterpart) -----------------------------
 * What closes a learner's loop behind ftgp_collect_values_device without a pass through the caller's framework: the gradient of the
 * clipped-PPO objective on rows of a collected rollout, with respect to every weight and bias of the slot's policy and of its value net,
 * and an Adam step on both in place -- in the buffers ftgp_set_net_device and ftgp_set_value_net_device write, so that the next launch
 * that names the slot runs the new network.
 *
 * The trainer of slot s.  ftgp_train_begin (host; may synchronise) gives a defined slot that has a value net and no population a
 * trainer: a gradient buffer and two moment buffers for each of the two nets, zeroed, a step count t = 0, and the scratch memory for
 * partial sums (256 sets of both gradients in the library's layout).  FTGP_ERR_STATE for a slot that is not defined, has no value net,
 * carries a population or has a trainer already; FTGP_ERR_ARG, naming the field, for a slot outside 0 .. 3, desc == NULL, beta1, beta2
 * or eps not finite, a beta outside [0, 1), eps <= 0, reserved != 0 -- everything is checked before anything changes.  ftgp_train_end
 * frees it (FTGP_ERR_STATE without one).  So do ftgp_destroy and the host setters that can change a shape: ftgp_set_net,
 * ftgp_set_net_frame, ftgp_set_net_rivals and ftgp_set_value_net on that slot, and a ftgp_set_net_population that gives it a population.
 * ftgp_set_net_device and ftgp_set_value_net_device replace parameters and leave the moments and t alone.  A handle that never calls
 * ftgp_train_begin allocates and launches exactly what it did before there were trainers.
 *
 * ftgp_train_grad_device only enqueues, ordered on `stream` exactly as ftgp_set_net_device.  It overwrites the trainer's gradient with
 * the gradient of L below at the parameters in force.  Batch row i = 0 .. n_batch-1 is row index[i] of the buffers, or first_row + i
 * with index == NULL; its weight w is weight[row], or 1; S = the sum of w over the batch rows.  A row number outside [0, n_rows)
 * contributes nothing, is counted in stats[6] and is never dereferenced; its new_mean and new_value entries are 0.
 * Per row, with x the row of inputs:
 *   y  = the slot's layers on x ("Layers" of "Network drivers", verbatim);  m_k = fmaf(y_k, out_scale[k], out_offset[k]);
 *        new_mean[i] = (m_0, m_1)
 *   yv = the value net's layers on x, likewise;  v = fmaf(yv, out_scale, out_offset);  new_value[i] = v
 *   p_k = std[k]*noise[row][k] + mean[row][k] (the action before the clip, step 1 of "Collected rollouts");  z_k = (p_k - m_k) / std[k]
 *   logp = -(z_0^2 + z_1^2)/2;  logq = -(noise_0^2 + noise_1^2)/2;  rho = exp(logp - logq)
 *   A = advantage[row];  s = min(rho*A, clamp(rho, 1-c, 1+c)*A), c = clip;
 *   ds/drho = A where (A >= 0 and rho <= 1+c) or (A < 0 and rho >= 1-c), else 0 -- evaluated as "0 where (A >= 0 and rho > 1+c) or
 *             (A < 0 and rho < 1-c), else A": comparisons with a NaN are false, so a NaN advantage or ratio is not clipped away, reaches
 *             the gradient and sets stats[5]
 *   L = -(1/S) sum w*s + value_coef * (1/S) sum w*(v - ret[row])^2/2
 * The derivative of an activation is taken from the layer's stored output o: identity 1; relu o > 0; tanh 1 - o*o, hence 0 where a
 * clamp of TANH binds.  With S = 0 (or not > 0) the gradient and the stats are zeros.
 * To the bit: the two forward passes, that is new_mean and new_value -- with unchanged parameters new_mean equals the mean
 * ftgp_collect_device recorded for an unfinished car and new_value the value.  Everything else is binary32 as the implementation orders
 * it, with these promises: z_k is evaluated as noise[row][k] + (mean[row][k] - m_k) / std[k], so that at unchanged parameters z_k is the
 * noise, rho is exactly 1 and stats[3] and stats[4] are exactly 0; and the result is deterministic -- the same call on the same buffers
 * gives the same bits on any stream at any load: no floating-point atomics reach the gradient or the stats, and the number and the
 * order of the partial sums follow from the shapes alone (rows in tiles of 32, or of 16 for the widest nets; tile g, g + G, .. to
 * workgroup g of G = min(tiles, 256); the workgroups' sums added g ascending, then divided by S).  The sums behind stats [1] .. [4] are
 * carried in binary64 along that order (each row's term is binary32) and rounded to binary32 once, after the division by S, so that what
 * a stat loses does not grow with n_batch; S and the gradient are binary32 sums.
 * stats: [0] S; [1] -sum w*s / S; [2] sum w*(v - ret)^2/2 / S; [3] sum w*(logq - logp) / S; [4] sum w*[|rho - 1| > c] / S; [5] 1 if an
 * element of either gradient is not finite, else 0; [6] the rows refused; [7] 0.
 * Errors, all before anything is enqueued: FTGP_ERR_STATE for a slot without a trainer; FTGP_ERR_ARG, naming the field, for a slot
 * outside 0 .. 3, n_batch < 1 or n_rows < 1, first_row < 0 or first_row + n_batch > n_rows (with index == NULL), std not finite or
 * <= 0, clip or value_coef not finite or < 0, reserved != 0, and a buffer that is NULL (index, noise, weight, stats, new_mean and
 * new_value may be), not device memory on the handle's device or too small.
 *
 * ftgp_train_adam_device only enqueues, with the same ordering.  The host advances t and rounds once from binary64: b1 = beta1,
 * b2 = beta2, omb1 = 1 - beta1, omb2 = 1 - beta2, a = lr / (1 - beta1^t), r = 1 / sqrt(1 - beta2^t).  Then per parameter p with
 * gradient g and moments m and v, binary32 with one rounding per written operation (sqrtf and / are IEEE):
 *     m = fmaf(b1, m, omb1 * g);  v = fmaf(b2, v, omb2 * (g * g));  d = fmaf(sqrtf(v), r, eps);  p = fmaf(-a, m / d, p)
 * -- torch's Adam without weight decay (ftgp_adam_step of csrc/ftgp_net.h) -- over the slot's policy and value parameters.  If the
 * gradient's non-finite flag (stats[5]) is set, p, m and v of both nets stay exactly as they were; t still advances.  The zero padding
 * of the library's layout stays zero.  lr not finite or < 0 is FTGP_ERR_ARG, no trainer FTGP_ERR_STATE.
 *
 * ftgp_train_get (host, synchronous): the gradient (FTGP_TRAIN_GRAD) or a moment (FTGP_TRAIN_M, FTGP_TRAIN_V) of both nets in the
 * caller's flat layout -- the counts of ftgp_get_net and ftgp_get_value_net -- and t.  Any pointer may be NULL.  FTGP_ERR_STATE without a
 * trainer, FTGP_ERR_ARG for an unknown `what`.  FTGP_TRAIN_RAW_GRAD and FTGP_TRAIN_RAW_PARAMS are debug reads for tests: the gradient,
 * or the parameters in force, of both nets exactly as they lie in device memory -- the library's layout of "Network populations": per
 * layer Wt[n_in][ld] with ld = n_out rounded up to 64, then b[ld]; (n_in + 1) * ld floats per layer -- so that the padding can be seen
 * to be zeros.
 * Memory: a trainer holds three copies of both nets in the library's layout and 256 more as partial sums -- about 28 MB for an
 * 85 -> 64 -> 64 pair, about 150 MB for the largest shape (256 -> 128 x 3) -- until ftgp_train_end. */
#define FTGP_TRAIN_STATS 8
typedef struct FtgpTrainDesc {           /* the optimiser of one slot */
    float beta1, beta2, eps;             /* finite; 0 <= beta < 1; eps > 0 */
    int32_t reserved;                    /* 0 */
} FtgpTrainDesc;
int ftgp_train_begin(FtgpEnv *env, int slot, const FtgpTrainDesc *desc);
int ftgp_train_end(FtgpEnv *env, int slot);

typedef struct FtgpTrainBatch {
    void *stream;                 /* as ftgp_set_net_device */
    int32_t slot;
    int32_t n_rows;               /* rows in the buffers below: T * n_envs * n_ext of the rollout */
    int32_t n_batch;              /* B >= 1 rows of this minibatch */
    int32_t first_row;            /* used when index == NULL: rows first_row .. first_row + B - 1 */
    const int32_t *index;         /* optional int32[B] row numbers, any order, repeats allowed */
    const float *inputs;          /* float32[n_rows][n_in] */
    const float *mean;            /* float32[n_rows][2]   Rollout.mean */
    const float *noise;           /* optional float32[n_rows][2]; NULL = zeros */
    const float *advantage, *ret; /* float32[n_rows] */
    const float *weight;          /* optional float32[n_rows] >= 0; NULL = ones */
    float std[2];                 /* > 0, finite */
    float clip;                   /* c >= 0, finite */
    float value_coef;             /* >= 0, finite */
    float *stats;                 /* optional float32[FTGP_TRAIN_STATS] */
    float *new_mean, *new_value;  /* optional float32[B][2], float32[B]: the forward pass on the batch rows */
    int32_t reserved[2];          /* 0 */
} FtgpTrainBatch;
int ftgp_train_grad_device(FtgpEnv *env, const FtgpTrainBatch *b);
int ftgp_train_adam_device(FtgpEnv *env, void *stream, int slot, float lr);
#define FTGP_TRAIN_GRAD 0
#define FTGP_TRAIN_M    1
#define FTGP_TRAIN_V    2
#define FTGP_TRAIN_RAW_GRAD   3   /* for tests: the gradient as it lies in device memory, the library's layout, padding included */
#define FTGP_TRAIN_RAW_PARAMS 4   /* for tests: likewise the slot's parameters in force */
int ftgp_train_get(FtgpEnv *env, int slot, int what, float *policy_out, float *value_out, int64_t *steps_out);

/* Read-backs (host buffers).  All are synchronous with respect to earlier calls on the handle. */

/* float[n_cars][n_rays]; replaces data.sensordata[vehicle_state.sensors] (custom.py:1395; drive.py:81).
 * Index 0 = rear, counter-clockwise; world units; -1 = no hit; all 0 right after reset, and all 0 for a car that has
 * finished (its rangefinders are switched off when it is sent to the shadow realm, custom.py:1436-1439). */
int ftgp_get_lidar(FtgpEnv *env, float *out);

/* double[n_cars][FTGP_SNAPSHOT_DOUBLES]; replaces VehicleState.snapshot (custom.py:149-160,62-76;
 * vehicle.py:3-12) incl. the reference's time = steps / timestep (custom.py:1397). */
int ftgp_get_snapshot(FtgpEnv *env, double *out);

/* double[n_cars][FTGP_POSE_DOUBLES]; replaces joint.qpos / joint.qvel reads (custom.py:1340; 149-152). */
int ftgp_get_pose(FtgpEnv *env, double *out);

/* int32[n_cars][FTGP_PROGRESS_INTS]; replaces the VehicleState race fields (custom.py:91-143,1340-1372).
 * finish_step orders the finishers of an env: the reference hands out places in the order cars reach lap_target, and within
 * one step in car order (winners[id] = len(winners) + 1 inside the per-car loop, custom.py:1337,1367-1369) -- i.e. by
 * (finish_step, car index).  It survives a multi-step ftgp_rollout, so one launch to the end of a race still says who won. */
int ftgp_get_progress(FtgpEnv *env, int32_t *out);

/* double[n_cars]: the squared distance to the nearest centre-line point as the progress block stored it last (custom.py:1343; off_track
 * is this > 1, custom.py:1344) -- the field entry 5 of a device state row is the square root of. */
int ftgp_get_centre_dist2(FtgpEnv *env, double *out);

/* float[n_cars][FTGP_CONTACT_FLOATS]: the contact row (see FTGP_CONTACT_FLOATS) of EVERY car at the current state; any handle. */
int ftgp_get_contacts(FtgpEnv *env, float *out);

/* float[n_cars][FTGP_FRAME_FIXED + 2*n_ahead]: the frame row (see FTGP_FRAME_FIXED) of EVERY car at the current state, with the
 * n_ahead (0 .. FTGP_MAX_LOOKAHEAD) and stride (1 .. 50) given here (FTGP_ERR_ARG otherwise); any handle. */
int ftgp_get_frames(FtgpEnv *env, int n_ahead, int stride, float *out);

/* float[n_cars][FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS*n_rivals]: the rival row (see FTGP_RIVAL_FIXED) of EVERY car at the current
 * state, with the n_rivals (0 .. FTGP_MAX_RIVALS) given here (FTGP_ERR_ARG otherwise); any handle. */
int ftgp_get_rivals(FtgpEnv *env, int n_rivals, float *out);

/* int32[n_cars]: place of each car among the finishers of its env, 1 = winner, 0 = still racing (Mujoco.winners, custom.py:1125,1367-1369). */
int ftgp_get_winners(FtgpEnv *env, int32_t *out);

/* counts: int32[n_cars] = len(VehicleState.times), the TRUE count; times: double[n_cars][FTGP_MAX_LAP_TIMES] = the ring of the newest
 * 32 (lap time k in slot k % 32, see FTGP_MAX_LAP_TIMES); replaces VehicleState.times (custom.py:124,1351-1363). */
int ftgp_get_lap_times(FtgpEnv *env, int32_t *counts, double *times);

/* int64[n_cars][2] = (start, finish_step): the env step of the car's last counted line crossing (vehicle_state.start, custom.py:1362) and
 * the env step at which `finished` was set (-1 while racing) with all 64 bits of self.steps; columns 6 and 9 of ftgp_get_progress hold the
 * same two saturated at 2^31 - 1. */
int ftgp_get_race_steps(FtgpEnv *env, int64_t *out);

/* double[n_cars][2] current controls. */
int ftgp_get_ctrl(FtgpEnv *env, double *out);

/* int64[n_envs] physics steps since each env's last reset (self.steps, custom.py:1124,1426). */
int ftgp_get_steps(FtgpEnv *env, int64_t *out);

/* Overwrite poses (testing / curriculum): double[n_cars][FTGP_POSE_DOUBLES]; only x, y, yaw (from qw, qz), vx, vy, wz are used. */
int ftgp_set_pose(FtgpEnv *env, const double *pose);

/* Evaluate a device policy once on caller-supplied scans: ranges float[n_cars][n_rays] replaces the stored scan,
 * the policy writes each car's controls (and fast.py's last_steering_angle); ctrl_out double[n_cars][2] (may be NULL).
 * Replaces one vehicle_state.driver.process_lidar(ranges) call per car (custom.py:1404). */
int ftgp_policy_eval(FtgpEnv *env, int policy, const float *ranges, double *ctrl_out);

/* Re-evaluate the lap-progress block (custom.py:1340-1372) at the current poses and step counts, without integrating.
 * ftgp_reset ends with this; use it after ftgp_set_pose. */
int ftgp_eval_progress(FtgpEnv *env);

/* Local metrics record (double[FTGP_METRIC_DOUBLES]) reduced on the device. */
int ftgp_metrics_local(FtgpEnv *env, double *out);

/*
 * Multi-GPU: one handle per rank, envs sharded, no data-path collective.
 * The only exchange is the end-of-step metrics all-gather over RCCL.
 *   ftgp_comm_unique_id : rank 0 creates the 128-byte RCCL id; the host ships it to the other ranks.
 *   ftgp_comm_init      : ncclCommInitRank on the handle's device.
 *   ftgp_metrics_allgather : out = double[world_size][FTGP_METRIC_DOUBLES]; runs on a side stream.
 * Nothing in the reference to mirror (it has no collective call sites).
 */
int ftgp_comm_unique_id(uint8_t id_out[128]);
int ftgp_comm_init(FtgpEnv *env, const uint8_t id[128], int rank, int world_size);
int ftgp_metrics_allgather(FtgpEnv *env, double *out);
/*
 * The same exchange in two halves, so that it overlaps the next launch ("side stream, overlapped with the
 * next step kernel"):
 *   ftgp_metrics_allgather_begin : enqueues, behind the most recent ftgp_step / ftgp_rollout launch, the all-gather of the
 *                                  record that launch leaves and the copy to pinned host memory -- on the side stream -- and
 *                                  returns at once.  The caller may launch the next steps right away.
 *   ftgp_metrics_allgather_end   : waits for that exchange only (never for a later launch) and copies the records out.
 * The step kernel writes its record into one of two slots, alternating per launch; a launch that would reuse the slot of an
 * exchange still in flight waits for it on the device.  At most one exchange may be open per handle (a second begin before
 * the end is FTGP_ERR_STATE); ftgp_metrics_allgather() == begin + end.
 */
int ftgp_metrics_allgather_begin(FtgpEnv *env);
int ftgp_metrics_allgather_end(FtgpEnv *env, double *out);

/*
 * fakelidar-compatible 2-D sphere tracing (ft_grandprix/raycast.py:5-21), batched over origins, one ray per lane.
 *   dt        double[H][W]   distance transform of the track image in pixels (the caller computes it, as the
 *                            reference does with scipy: custom.py:1149-1153, raycast.py:24-27)
 *   origins   double[n_origins][2]   (orig_x, orig_y) in pixels
 *   cosines / sines  double[n_origins][rangefinders]
 *   scan      double[n_origins][rangefinders]        accumulated distance per ray (pixels)
 *   points    double[n_origins][rangefinders][2]     end point per ray
 * Same loop as the reference: while dt[int(y), int(x)] > eps and 0 <= x <= W and 0 <= y <= H: advance by dt.
 * int() truncates toward zero and negative indices wrap like numpy's; an index past the end (>= W / H) or below -W / -H
 * is the reference's IndexError and is reported as FTGP_ERR_ARG.  A ray whose lookup was valid ends without error once
 * x < 0 or y < 0.  Standalone: needs no FtgpEnv.
 */
int ftgp_fakelidar(int device_id, const double *dt, int H, int W, int n_origins, const double *origins, int rangefinders,
                   const double *cosines, const double *sines, double eps, double *scan, double *points);

/* FAKELIDAR mode: the distance transform ftgp_create built, double[height][width] in pixels (what the reference calls self.dt,
 * custom.py:1152-1153); FTGP_ERR_STATE in RANGEFINDER mode and on a handle with more than one track. */
int ftgp_get_distance_field(FtgpEnv *env, double *out);

/* FAKELIDAR mode: the distance transform of track `track` (0 .. n_tracks - 1) of a handle, double[height][width] of that track; any
 * handle (one made by ftgp_create has track 0).  FTGP_ERR_ARG for a track out of range, FTGP_ERR_STATE in RANGEFINDER mode. */
int ftgp_get_track_distance_field(FtgpEnv *env, int track, double *out);

/* Self-test of device arithmetic the kernels rely on (no reference counterpart): the fast reciprocal of the ray set-up against
 * the IEEE division of the specification over all 2^32 binary32 bit patterns.  *mismatches = number of differing results. */
int ftgp_selftest(int device_id, int64_t *mismatches);

/* Timing of the most recent ftgp_step / ftgp_rollout launch sequence, measured with HIP events on the handle's stream (ms). */
int ftgp_last_kernel_ms(FtgpEnv *env, float *ms);

/* Name of the kernel that ftgp_rollout/ftgp_step launches for the current configuration (for rocprof matching). */
const char *ftgp_kernel_name(FtgpEnv *env);

/* What the loaded library was built from and with (no reference counterpart; touches no device):
 * "abi=<n> sources=<hash of the kernel sources, tools/evidence.py sha> diag=<diagnostic switches, "none" in the product> fair_shift=<n>
 * waves_per_eu=<n>".  __graft_entry__.build() rebuilds a library whose hash is not the tree's; tests/test_capi.py checks both fields. */
const char *ftgp_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* FTGP_H */
