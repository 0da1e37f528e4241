// ftgp_kernels.hip -- HIP kernels of the ft_grandprix hot path for gfx950 (CDNA4, wave64).
//
//   ftgp_step_kernel<MULTI, FAKE, ROSTER, TRACKS>   n_steps per launch; one workgroup = whole envs, up to 16 cars on up to 16 waves (the headline
//       shape is 8 cars on 16 waves, two workgroups per CU), persistent over all steps.  ONE workgroup barrier per step.  Inside a
//       step, concurrently:
//         K5       waves 0 .. cars-1, one car each: the driver on the car's PREVIOUS scan (the other LDS scan buffer) -> controls
//         K1 + K3  the wave whose driver delivers last: integrate + lap progress for ALL cars of the workgroup on four lanes per
//                  car (dynamics_lanes), then the LiDAR frames of the NEXT step into the other frame buffer
//         K2       every wave, as soon as its driver work is done: the sweep of THIS step in groups of 64 neighbouring rays of one car
//                  (lidar_groups): a wave draws a task -- a group, or a group and the same rays turned round --, sets the rays up,
//                  marches them until all have finished (march_all, hand-written) and delivers the 64 ranges: one 256-byte segment of
//                  the car's row in HBM, the drivers' window also into the LDS scan buffer.
//       The sweep reads the LiDAR frames, never the live state, and the scan a driver sees lags the pose by one step
//       (custom.py:1395-1425): that is what makes the overlap legal.
//       Staged into LDS once per launch, in one pass, from an image laid out as the LDS is: parameter block, vehicle constants,
//       centre-line, ray table, cover tables; then the cars' state records and the scan windows the drivers read.  The march reads the
//       sector box field from L2 (ftgp_march.h).  FAKE: K2 is the reference's own 2-D LiDAR (lidar_fake).  ROSTER: every car slot its own driver.
//       The end-of-launch metrics record is part of the kernel (launch_metrics).
//       TRACKS: multi-track handles (ftgp_create_tracks) -- each workgroup looks up its track and first car at entry, then stages and races that track.
//   ftgp_policy_kernel    K5 alone (ftgp_policy_eval).
//   ftgp_collect_act_kernel  the network of a slot for every external car, one wave each: inputs, mean and action of a collected decision.
//   ftgp_reset_kernel     K4 reset / spawn (+ K3 at the spawn pose), one car per lane.
//   ftgp_progress_kernel  K3 alone (after ftgp_set_pose), one car per lane.
//   ftgp_fakelidar_kernel raycast.fakelidar restated, one ray per lane.
//   ftgp_box_field_kernel the sector box field at create; ftgp_edt_kernel the distance transform of FAKELIDAR mode.
//   ftgp_metrics_kernel   per-GPU metrics record.
//
// Reference behaviour restated by each block is cited inline (paths relative to the reference repo).
// Arithmetic follows DESIGN.md operation by operation (-ffp-contract=off; fmaf only where the specification
// says "fma"), so results are bit-identical to the CPU oracle.
#include "ftgp_device.h"

// K1 staging types
struct Force { double fx, fy, tz; };
struct Dyn { double x, y, qw, qz, vx, vy, wz, qs, qsd, w[4]; };
static_assert(sizeof(Dyn) == 104 && offsetof(CarCore, w) == offsetof(Dyn, w) && offsetof(CarCore, qsd) == offsetof(Dyn, qsd), "Dyn must mirror the head of CarCore");
#define FTGP_FORCE_TERMS 11      // 4 wheels, 3 chassis circles, 4 softeners: summed in this order

struct Lds {
    const VehLds* veh;
    const double* path;
    const float2* ray;        // body-frame ray directions
    CarCore* cars;
    LidarFrame* frame;        // [2][cars_per_block], double-buffered by step parity
    PairCull* pairs;          // [2][cars_per_block][FTGP_PAIR_STRIDE], right behind the frames (multi-car envs only)
    int64_t* steps;
    float* scan;              // [2][cars_per_block][win_floats] scan windows (layout: scan_window_* below), double-buffered by step parity
    int* list;                // [waves_per_block][64] driver scratch
    int* pool;                // [2] next ray group of the sweep (lidar_groups), [2] drivers finished, [2] "some LiDAR frame is
                              // not known to lie well inside the image" (frame_write) -- all double-buffered by step parity
    Force* terms;             // [cars_per_block][FTGP_FORCE_TERMS] K1 staging: force terms in the order they are summed
    double* wnew;             // [cars_per_block][4] K1 staging: new wheel spins
    Dyn* next;                // [cars_per_block] K1 staging: new dynamic state before the commit
    Force* mates;             // [cars_per_block][FTGP_PAIR_STRIDE] K1 staging, multi-car envs: the contact forces with each env-mate, summed (car_contact_mate)
    const float* cover;       // [cover_kmax + 1] cover-count thresholds of the launch's driver (see cover_count)
    unsigned char* mmask;     // [2][cars_per_block][mmask_stride] multi-car envs: which env-mates each ray group of a car can see (mate_masks)
};

// LDS scan window of one car: the samples the on-device drivers read.  Sample ranges[eighth + i] sits at float index
// (eighth % 4) + i, so that LDS and HBM addresses of a sample agree modulo 16 bytes (whole float4 groups move with one
// ds_read_b128 + one global_store_dwordx4); ranges[0] (fast.py:135) sits in the last float of the row.
__device__ __forceinline__ int scan_window_first(int eighth) { return eighth & 3; }

// A wave-uniform value the optimiser cannot see through.  The step loop rebuilds its LDS pointers from such offsets every
// step, so loads of constants (vehicle parameters, centre-line, ...) are never hoisted out of the loop -- hoisted, they
// would stay live across the sweep and end up in scratch memory under the 64-VGPR budget.
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+s"(v)); return v; }
// The parameter block as the scalar unit sees it: the kernel argument's copy in device memory, read through the constant address
// space, i.e. with scalar loads -- wave-uniform values then reach their SGPRs without a vector instruction (out of LDS each one
// costs a read and a v_readfirstlane, out of a spilled SGPR a v_readlane: the vector pipe is what this kernel is short of).
// The pointer is made opaque once per step, so the loads stay inside the step instead of being hoisted and spilled.
typedef const __attribute__((address_space(4))) DeviceParams* ScalarParams;
__device__ __forceinline__ ScalarParams scalar_view(const DeviceParams* p)
{
    uint64_t a = (uint64_t)p; asm volatile("" : "+s"(a));
    return (ScalarParams)a;
}
// the lane index, recomputed where it is used: values derived from it (per-lane addresses, selects) then stay local to the phase
// that needs them instead of being hoisted in front of the step loop and carried -- spilled -- across the sweep
__device__ __forceinline__ int lane_here() { int l = lane_id(); asm volatile("" : "+v"(l)); return l; }

struct LdsOffsets { int params, veh, path, ray, cars, frame, steps, scan, list, pool, k1, cover, mmask, cpb; };

__device__ __forceinline__ LdsOffsets lds_offsets(const DeviceParams& P)
{
    LdsOffsets o;
    o.params = sgpr(P.off_params); o.veh = sgpr(P.off_veh); o.path = sgpr(P.off_path); o.ray = sgpr(P.off_ray); o.cars = sgpr(P.off_cars);
    o.frame = sgpr(P.off_frame); o.steps = sgpr(P.off_steps); o.scan = sgpr(P.off_scan); o.list = sgpr(P.off_list); o.pool = sgpr(P.off_pool);
    o.k1 = sgpr(P.off_k1); o.cover = sgpr(P.off_cover); o.mmask = sgpr(P.off_mmask); o.cpb = sgpr(P.cars_per_block);
    return o;
}

__device__ __forceinline__ LdsOffsets lds_offsets(ScalarParams G)
{
    LdsOffsets o;
    o.params = G->off_params; o.veh = G->off_veh; o.path = G->off_path; o.ray = G->off_ray; o.cars = G->off_cars;
    o.frame = G->off_frame; o.steps = G->off_steps; o.scan = G->off_scan; o.list = G->off_list; o.pool = G->off_pool;
    o.k1 = G->off_k1; o.cover = G->off_cover; o.mmask = G->off_mmask; o.cpb = G->cars_per_block;
    return o;
}

// what the on-device drivers need to know about the scan (wave-uniform)
struct DriverShape { int n_rays, eighth, win_floats, cover_kmax; double rpp; float two_over_rpp; };
template <class PP> __device__ __forceinline__ DriverShape driver_shape(PP p)
{
    DriverShape d; d.n_rays = p->n_rays; d.eighth = p->eighth; d.win_floats = p->win_floats; d.cover_kmax = p->cover_kmax; d.rpp = p->rpp; d.two_over_rpp = p->two_over_rpp;
    return d;
}

__device__ __forceinline__ Lds lds_view(const LdsOffsets& o, unsigned char* lds)
{
    Lds L;
    L.veh = reinterpret_cast<const VehLds*>(lds + opaque(o.veh));
    L.path = reinterpret_cast<const double*>(lds + opaque(o.path));
    L.ray = reinterpret_cast<const float2*>(lds + opaque(o.ray));
    L.cars = reinterpret_cast<CarCore*>(lds + opaque(o.cars));
    L.frame = reinterpret_cast<LidarFrame*>(lds + opaque(o.frame));
    L.pairs = reinterpret_cast<PairCull*>(L.frame + 2 * o.cpb);
    L.steps = reinterpret_cast<int64_t*>(lds + opaque(o.steps));
    L.scan = reinterpret_cast<float*>(lds + opaque(o.scan));
    L.list = reinterpret_cast<int*>(lds + opaque(o.list));
    L.pool = reinterpret_cast<int*>(lds + opaque(o.pool));
    unsigned char* k1 = lds + opaque(o.k1);     // one block: terms | wnew | next (sizes follow from cars_per_block)
    L.terms = reinterpret_cast<Force*>(k1);
    L.wnew = reinterpret_cast<double*>(k1 + o.cpb * (int)(FTGP_FORCE_TERMS * sizeof(Force)));
    L.next = reinterpret_cast<Dyn*>(k1 + o.cpb * (int)(FTGP_FORCE_TERMS * sizeof(Force) + 4 * sizeof(double)));
    L.mates = reinterpret_cast<Force*>(k1 + o.cpb * (int)(FTGP_FORCE_TERMS * sizeof(Force) + 4 * sizeof(double) + sizeof(Dyn)));
    L.cover = reinterpret_cast<const float*>(lds + opaque(o.cover));
    L.mmask = lds + opaque(o.mmask);
    return L;
}

// =============================================================================================
// K2: LiDAR
// =============================================================================================
// The sweep of one step for all cars of the workgroup, executed by every wave.  Rangefinder geometry:
// template/mushr.em.xml:98-117 -- ray j leaves the ring at centre - 0.03*dir_j, dir_j = R(yaw) * (sin phi_j, -cos phi_j);
// j = 0 is the rear, CCW.  Values replace data.sensordata[vehicle_state.sensors] (custom.py:1395).
//
// Scheduling: lidar_groups() below -- groups of 64 neighbouring rays, march_all().  Which lane marches which ray has no influence on any result.
// number of set bits of `mask` below this lane
__device__ __forceinline__ int rank_below(uint64_t mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0)); }

// |1 / x| and |1 / y| correctly rounded, as the specification's IEEE divisions give them.  One Newton step on v_rcp_f32
// (1 ulp) with fused residuals is correctly rounded for every binary32 input with 2^-100 < |x| < 2^100 (checked exhaustively
// over all 2^32 bit patterns by ftgp_selftest / tests/test_gpu_parity.py); zeros, denormals, huge values and NaNs take the
// division.  The range test is done on the bit patterns of both operands at once: b - (lo + 1) is below hi - lo - 1 (unsigned)
// exactly for lo < b < hi, and the OR of two such differences can only be below that if both are -- an OR that is not sends
// the wave through the per-lane test and the division, which is then simply not needed.
// CLAMP: +inf (a zero, or so small that its reciprocal overflows) comes back as FTGP_IV_MAX, as the ray specification wants it.
template <bool CLAMP = false>
__device__ __forceinline__ void rcp_abs2(float x, float y, float& rx, float& ry)
{
    const float ax = fabsf(x), ay = fabsf(y);
    float p = __builtin_amdgcn_rcpf(ax), q = __builtin_amdgcn_rcpf(ay);
    const float ep = fmaf(-ax, p, 1.0f), eq = fmaf(-ay, q, 1.0f);
    p = fmaf(p, ep, p); q = fmaf(q, eq, q);
    // (the patterns doubled: the shift drops the sign, so dropping it and subtracting is one shift-add per operand, not an AND and an add)
    const uint32_t lo1 = 2u * 0x0D800001u, span = 2u * (0x71800000u - 0x0D800001u);             // bit patterns of 2^-100 (+ 1) and 2^100, twice
    if (__any((((__float_as_uint(x) << 1) - lo1) | ((__float_as_uint(y) << 1) - lo1)) >= span)) {
        const bool oddx = !(ax > 0x1p-100f && ax < 0x1p100f), oddy = !(ay > 0x1p-100f && ay < 0x1p100f);      // also true for a NaN
        float zx = fabsf(1.0f / x), zy = fabsf(1.0f / y);
        if (CLAMP) { zx = zx < FTGP_IV_MAX ? zx : FTGP_IV_MAX; zy = zy < FTGP_IV_MAX ? zy : FTGP_IV_MAX; }
        p = oddx ? zx : p; q = oddy ? zy : q;
    }
    rx = p; ry = q;
}

// Ray against another car: chassis box (slab test) and LiDAR puck (circle; left out where it cannot win, VehLds::puck_in_box), binary32 -- the specification's arithmetic with
// everything that does not depend on the ray taken from where it already exists: (bx, by) = mate's origin - my LiDAR centre is
// the pair record's (its negation is the specification's (float)(centre - origin): binary64 subtraction and the conversion
// are odd functions), the mate's heading in binary32 is its LiDAR frame's, the vehicle constants in binary32 are VehLds',
// and the two IEEE reciprocals are rcp_abs2's with the sign put back.
__device__ __forceinline__ float ray_vs_car(const VehLds* V, const LidarFrame* b, float bx, float by, float dxw, float dyw)
{
    const float r0 = V->ring_radius_f;
    float best = INFINITY;
    const float relx = -bx, rely = -by;
    const float ox = fmaf(dxw, -r0, relx), oy = fmaf(dyw, -r0, rely);
    const float cbf = b->chf, sbf = b->shf;
    const float lx = fmaf(cbf, ox, sbf * oy), ly = fmaf(cbf, oy, -(sbf * ox));
    const float ldx = fmaf(cbf, dxw, sbf * dyw), ldy = fmaf(cbf, dyw, -(sbf * dxw));
    {
        const float xmin = V->box_xmin_f, xmax = V->box_xmax_f, ymin = V->box_ymin_f, ymax = V->box_ymax_f;
        float tmin = -INFINITY, tmax = INFINITY; bool miss = false;
        float ax, ay;
        rcp_abs2(ldx, ldy, ax, ay);
        if (ldx != 0.0f) {
            const float inv = copysignf(ax, ldx); const float t1 = (xmin - lx) * inv, t2 = (xmax - lx) * inv;
            tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
        } else if (lx < xmin || lx > xmax) miss = true;
        if (ldy != 0.0f) {
            const float inv = copysignf(ay, ldy); const float t1 = (ymin - ly) * inv, t2 = (ymax - ly) * inv;
            tmin = fmaxf(tmin, fminf(t1, t2)); tmax = fminf(tmax, fmaxf(t1, t2));
        } else if (ly < ymin || ly > ymax) miss = true;
        if (!miss && tmax >= fmaxf(tmin, 0.0f)) {
            const float t = tmin > 0.0f ? tmin : 0.0f;
            if (t < best) best = t;
        }
    }
    if (!sgpr(V->puck_in_box)) {            // (wave-uniform; with the puck inside the box -- both bundled vehicles -- the box's time is the minimum already: VehLds)
        const float px = lx - V->lidar_x_f, py = ly - V->lidar_y_f;
        const float bq = fmaf(px, ldx, py * ldy);
        const float cq = fmaf(px, px, py * py) - r0 * r0;
        const float disc = fmaf(bq, bq, -cq);
        if (disc >= 0.0f) {
            float t = -bq - sqrtf(disc);
            if (t < 0.0f) t = (cq < 0.0f) ? 0.0f : INFINITY;
            if (t < best) best = t;
        }
    }
    return best;
}

// Measurement hooks (phase stamps, workgroup entry / exit times, phases compiled out): all of them live in diag/ftgp_diag.inc and exist only
// in libraries built with -DFTGP_DIAG by tools/*.sh on the GPU box.  The product build defines none of them (ftgp_build_info() says so,
// tests/test_capi.py checks it).
#include "diag/ftgp_diag.inc"

// Two workgroups share a CU, and the hardware arbitrates vector issue by priority first and age second: left alone, the
// workgroup that was dispatched first wins every contested cycle, finishes a launch ~20 % ahead of its partner and leaves the CU
// half empty (four waves per SIMD, too few to keep the vector pipe full) for the rest of it.  So the two take turns: a 100-MHz
// wall-clock bit that both see picks which of them sweeps at the raised priority.  "Workgroups b and b + (number of CUs) are
// partners" is only what the dispatcher is observed to do (the hardware promises no order); a wrong guess costs fairness,
// never correctness.
#ifndef FTGP_FAIR_SHIFT
#define FTGP_FAIR_SHIFT 14        // turns of 2^14 ticks = 164 us (round 3: 2^12 .. 2^15 equally good; on round 5's kernel 2^14 is 1.2 % ahead of 2^13 in sixteen same-box rows,
                                  // 2^11, 2^12 and 2^15 behind: profiles/round5/ab_fair_turns.log)
#endif
__device__ __forceinline__ void sweep_priority(bool second_half)
{
    if (!FTGP_DIAG_FAIR) return;
    const bool mine = (((uint32_t)__builtin_amdgcn_s_memrealtime() >> FTGP_FAIR_SHIFT) & 1u) != (second_half ? 1u : 0u);
    if (mine) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
}

// The march of one wave's rays until ALL of them sit on their terminal cell: hand-written, for two reasons that round 5 measured one after the other
// (DESIGN.md section 6).  (1) Instruction count: scalar, branch and wait instructions cost a SIMD about what a cheap vector instruction costs
// (profiles/round4/salu_cost.log), and the compiler's loop spends 13 scalar-side instructions per iteration on mask bookkeeping.  Here a lane leaves the
// loop by dropping out of exec (v_cmpx on "the cell's entry is a box", i.e. kx != 0), so the body needs no live mask, finished rays hold their crossing
// times for free (and burn no vector lanes), and an iteration is 20 vector (the look-up's six included) + 3 scalar-side instructions, + the near-boundary path;
// the crossing time into the terminal cell is the smaller of the last jump's two, taken once after the loop.
// (2) The dependent chain from one look-up to the next, which is what the waves spend most of their life on: the next look-up is issued as soon as the
// landing estimate's floor is there; the near-boundary test (fract, recentre, compare, branch) runs in the load's shadow, and a
// lane that turns out to be within eps of a pixel boundary recomputes its cell (ftgp_ray_fix) and looks up again -- answers return in order, the second
// overwrites the first.  For the fix path to find the cell the ray came from after the move has been made, the loop runs two iterations per trip with the
// cell alternating between (mx, my) and (nx, ny).  The first look-up and jump are peeled (the start cell is (0, 0): no zeroes to set, a mask and a shift
// for the byte-select adds), and the tail of ftgp_ray_place -- g, the origin's offset inside its start cell seen in the direction of travel, and c = g * iv --
// is worked out in the shadow of that first load.  (-5.4 % and -1.1 % of the headline's cycles: profiles/round5/ab_speculative_lookup.log,
// ab_setup_latency_experiments.log.)
// In: exec = the lanes that hold a ray; (pu, pv) = the ray's origin in pixels (on the image, or the ray is parked: base = 0, ax = ay = 0), du, dv signed
// (the body reads their magnitudes through the operand modifier), ivx, ivy = |1 / du|, |1 / dv| as the specification wants them, base = the byte offset
// of the start cell's entry, ax, ay = the strides.
// Out: w = the terminal cell's entry (0 = wall, FTGP_FIELD_OUT = ring), s = the crossing time into it; exec as on entry.
// The arithmetic is ftgp_ray_place's tail and ftgp_ray_step / ftgp_ray_fix / ftgp_ray_commit of ftgp_march.h, instruction for instruction: a crossing
// time is fma((float)boundary, iv, -c) -- boundaries counted from the ray's own start cell.
__device__ __forceinline__ void march_all(float& s, uint32_t& w, float pu, float pv, float ivx, float ivy, float du, float dv,
                                          int base, int ax, int ay, float thr /* 0.5f - eps */, const void* field)
{
    int a, b, c, d, e, f, h, i, mx, my, nx, ny;
    float gu, gv, cx, cy;
    uint64_t stepx, sv, sq, ex0;
    asm volatile(
        "s_mov_b64 %[ex0], exec\n\t"
        // crossing times of the box's far edges, the axis that is reached first, the landing estimate and its floor
#define FTGP_MARCH_BODY \
        "v_cvt_f32_i32_e32 %[a], %[c]\n\t" \
        "v_cvt_f32_i32_e32 %[b], %[d]\n\t" \
        "v_fma_f32 %[a], %[a], %[ivx], -%[cx]\n\t"                       /* sX = fma((float)xe, ivx, -cx): the box's far edge is the xe-th boundary */ \
        "v_fma_f32 %[b], %[b], %[ivy], -%[cy]\n\t"                       /* sY */ \
        "v_cmp_lt_f32_e64 %[stepx], %[a], %[b]\n\t"                      /* the x edge of the box is reached first (a tie steps in y) */ \
        "v_fma_f32 %[e], |%[dv]|, %[a], %[gv]\n\t"                       /* landing estimate after an x-jump ... */ \
        "v_fma_f32 %[f], |%[du]|, %[b], %[gu]\n\t"                       /* ... after a y-jump */ \
        "v_cndmask_b32_e64 %[e], %[f], %[e], %[stepx]\n\t"               /* v */ \
        "v_cvt_flr_i32_f32_e32 %[h], %[e]\n\t"                           /* t = floor(v) */
        // the new cell (NX, NY) and its look-up, issued on the landing estimate; THEN the estimate's distance from a pixel boundary, in the shadow of
        // the load: within eps the specification's comparisons decide (fix) and the look-up is issued again for those lanes
#define FTGP_MARCH_MOVE(NX, NY, fix) \
        "v_cndmask_b32_e64 " NX ", %[h], %[c], %[stepx]\n\t" \
        "v_cndmask_b32_e64 " NY ", %[d], %[h], %[stepx]\n\t" \
        "v_mad_i32_i24 %[i], " NY ", %[ay], %[base]\n\t"                 /* entry offset = ftgp_ray_offset() */ \
        "v_mad_i32_i24 %[i], " NX ", %[ax], %[i]\n\t" \
        "global_load_ushort %[w], %[i], %[field]\n\t" \
        "v_fract_f32_e32 %[f], %[e]\n\t" \
        "v_add_f32_e32 %[f], -0.5, %[f]\n\t" \
        "v_cmp_gt_f32_e64 vcc, |%[f]|, %[thr]\n\t" \
        "s_cbranch_vccnz " fix "\n"
        // the entry of the cell the ray stands on: far corner of its box; kx == 0 -- a wall or ring cell -- and the lane is done
#define FTGP_MARCH_ARRIVE(NX, NY) \
        "s_waitcnt vmcnt(0)\n\t" \
        "v_add_u32_sdwa %[c], " NX ", %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"     /* xe = mx + kx */ \
        "v_add_u32_sdwa %[d], " NY ", %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\t"     /* ye = my + ky */ \
        "v_cmpx_ne_u32_e32 vcc, %[c], " NX "\n\t"
        // ftgp_ray_fix() for the lanes in vcc; cur = the select that yields the transverse coordinate of the cell the ray stands on
#define FTGP_MARCH_FIX(cur, NX, NY, back) \
        "s_and_saveexec_b64 %[sv], vcc\n\t" \
        "v_cndmask_b32_e64 %[s], %[cx], %[cy], %[stepx]\n\t"             /* transverse c ... (s, f, i, h: scratch here -- sX, sY stay: the crossing time is their minimum, taken after the loop) */ \
        "v_cndmask_b32_e64 %[f], %[ivx], %[ivy], %[stepx]\n\t"           /* ... reciprocal */ \
        "v_rndne_f32_e32 %[e], %[e]\n\t"                                 /* the boundary in doubt */ \
        "v_fma_f32 %[s], %[e], %[f], -%[s]\n\t"                          /* its crossing time, the specification's way */ \
        "v_cvt_i32_f32_e32 %[f], %[e]\n\t" \
        "v_min_f32_e32 %[h], %[a], %[b]\n\t"                             /* sn, the crossing time of the jump */ \
        "v_cmp_lt_f32_e64 vcc, %[s], %[h]\n\t" \
        "v_cmp_le_f32_e64 %[sq], %[s], %[h]\n\t" \
        "s_and_b64 %[sq], %[sq], %[stepx]\n\t"                           /* crossed: S <= sn after an x-jump, S < sn after a y-jump */ \
        "s_or_b64 vcc, vcc, %[sq]\n\t" \
        "v_cndmask_b32_e64 %[s], -1, 0, vcc\n\t" \
        "v_add_u32_e32 %[h], %[f], %[s]\n\t"                             /* the cell beyond the boundary if crossed, else the one before */ \
        cur                                                              /* the cell the ray stands on (transverse coordinate, into f) ... */ \
        "v_cndmask_b32_e64 %[i], %[c], %[d], %[stepx]\n\t" \
        "v_add_u32_e32 %[i], -1, %[i]\n\t"                               /* ... and the last cell of the box's span */ \
        "v_med3_i32 %[h], %[h], %[f], %[i]\n\t"                          /* inside the box's span */ \
        "v_cndmask_b32_e64 " NX ", %[h], %[c], %[stepx]\n\t"             /* the cell and its look-up again (the first look-up's answer arrives first and is overwritten) */ \
        "v_cndmask_b32_e64 " NY ", %[d], %[h], %[stepx]\n\t" \
        "v_mad_i32_i24 %[i], " NY ", %[ay], %[base]\n\t" \
        "v_mad_i32_i24 %[i], " NX ", %[ax], %[i]\n\t" \
        "global_load_ushort %[w], %[i], %[field]\n\t" \
        "s_mov_b64 exec, %[sv]\n\t" \
        "s_branch " back "\n"
        // The start cell and the first jump, peeled: the ray stands on cell (0, 0), so the box's far corner is the entry's two bytes as they
        // come (a mask and a shift for two byte-select adds) and nobody has to set the cell to zero first.
        "global_load_ushort %[w], %[base], %[field]\n\t"
        // ... and in the shadow of that load what the jumps need of the ray's origin (the tail of ftgp_ray_place): its offset inside the start cell seen in
        // the direction of travel, g, and c = g * iv; the crossing time into the start cell is 0
        "v_fract_f32_e32 %[gu], %[pu]\n\t"                               // p - floor(p): exact for every p >= 0 (an origin off the image is parked: it ends on this look-up)
        "v_fract_f32_e32 %[gv], %[pv]\n\t"
        "v_sub_f32_e32 %[a], 1.0, %[gu]\n\t"
        "v_sub_f32_e32 %[b], 1.0, %[gv]\n\t"
        "v_cmp_gt_f32_e32 vcc, 0, %[du]\n\t"                             // (a component of -0 counts as not negative: it never steps)
        "v_cndmask_b32_e32 %[gu], %[gu], %[a], vcc\n\t"
        "v_cmp_gt_f32_e32 vcc, 0, %[dv]\n\t"
        "v_cndmask_b32_e32 %[gv], %[gv], %[b], vcc\n\t"
        "v_mul_f32_e32 %[cx], %[gu], %[ivx]\n\t"
        "v_mul_f32_e32 %[cy], %[gv], %[ivy]\n\t"
        "v_mov_b32_e32 %[a], 0\n\t"                                      // (a ray that ends on its start cell: its crossing time is min(0, 0))
        "v_mov_b32_e32 %[b], 0\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "v_and_b32_e32 %[c], 0xff, %[w]\n\t"                              // xe = kx
        "v_lshrrev_b32_e32 %[d], 8, %[w]\n\t"                             // ye = ky
        "v_cmpx_ne_u32_e32 vcc, 0, %[c]\n\t"                              // kx == 0: the ray starts in a wall (or was parked on a ring cell)
        "s_cbranch_execz L_march_done_%=\n\t"
        FTGP_MARCH_BODY
        FTGP_MARCH_MOVE("%[mx]", "%[my]", "L_march_fix0_%=")
        "L_march_arrive0_%=:\n\t"
        FTGP_MARCH_ARRIVE("%[mx]", "%[my]")
        "s_cbranch_execz L_march_done_%=\n"
        // the loop, two iterations per trip: the cell alternates between (mx, my) and (nx, ny), so that the near-boundary path still finds the
        // cell the ray came from after the move has been made
        "L_march_loop_%=:\n\t"
        FTGP_MARCH_BODY
        FTGP_MARCH_MOVE("%[nx]", "%[ny]", "L_march_fix1_%=")
        "L_march_arrive1_%=:\n\t"
        FTGP_MARCH_ARRIVE("%[nx]", "%[ny]")
        "s_cbranch_execz L_march_done_%=\n\t"
        FTGP_MARCH_BODY
        FTGP_MARCH_MOVE("%[mx]", "%[my]", "L_march_fix2_%=")
        "L_march_arrive2_%=:\n\t"
        FTGP_MARCH_ARRIVE("%[mx]", "%[my]")
        "s_cbranch_execnz L_march_loop_%=\n\t"
        "s_branch L_march_done_%=\n"
        "L_march_fix0_%=:\n\t"
        FTGP_MARCH_FIX("v_mov_b32_e32 %[f], 0\n\t", "%[mx]", "%[my]", "L_march_arrive0_%=")
        "L_march_fix1_%=:\n\t"
        FTGP_MARCH_FIX("v_cndmask_b32_e64 %[f], %[mx], %[my], %[stepx]\n\t", "%[nx]", "%[ny]", "L_march_arrive1_%=")
        "L_march_fix2_%=:\n\t"
        FTGP_MARCH_FIX("v_cndmask_b32_e64 %[f], %[nx], %[ny], %[stepx]\n\t", "%[mx]", "%[my]", "L_march_arrive2_%=")
        "L_march_done_%=:\n\t"
        "s_mov_b64 exec, %[ex0]\n\t"
        "v_min_f32_e32 %[s], %[a], %[b]"                                  // the crossing time into the terminal cell: the smaller of the last jump's two (a finished lane's stay as they were)
        : [s] "=&v"(s), [w] "=&v"(w), [mx] "=&v"(mx), [my] "=&v"(my), [nx] "=&v"(nx), [ny] "=&v"(ny),
          [a] "=&v"(a), [b] "=&v"(b), [c] "=&v"(c), [d] "=&v"(d), [e] "=&v"(e), [f] "=&v"(f), [h] "=&v"(h), [i] "=&v"(i),
          [gu] "=&v"(gu), [gv] "=&v"(gv), [cx] "=&v"(cx), [cy] "=&v"(cy),
          [stepx] "=&s"(stepx), [sv] "=&s"(sv), [sq] "=&s"(sq), [ex0] "=&s"(ex0)
        : [pu] "v"(pu), [pv] "v"(pv), [ivx] "v"(ivx), [ivy] "v"(ivy), [du] "v"(du), [dv] "v"(dv),
          [base] "v"(base), [ax] "v"(ax), [ay] "v"(ay), [thr] "s"(thr), [field] "s"(field)
        : "vcc", "scc", "memory");
#undef FTGP_MARCH_BODY
#undef FTGP_MARCH_MOVE
#undef FTGP_MARCH_ARRIVE
#undef FTGP_MARCH_FIX
}

// A GATHER task of the window-only table (kind 3, plan_window_table): what a car's whole pairs and single groups leave over -- ray 0, the ends
// of the sideways zone and of the forward cone -- marched together.  Its lanes hold a few runs of consecutive rays; the runs of gather q come
// as ONE 16-byte scalar load from behind the table's draws (`gathers`), a word each: (first ray - first lane) & 0xffff | first lane << 16, a
// run the task does not have starting at lane 64.  field: the draw's first-ray field, lanes | q << 7.  Shared by lidar_groups and lidar_fake.
template <class ScalarTasksT>
__device__ __forceinline__ void gather_lanes(ScalarTasksT gathers, int field, int lane, int& j, bool& mine)
{
    const uint32_t q = (uint32_t)field >> 7;
    const int r0 = gathers[q].x, r1 = gathers[q].y, r2 = gathers[q].z, r3 = gathers[q].w;
    int d = (int16_t)r0;
    if (lane >= (r1 >> 16)) d = (int16_t)r1;
    if (lane >= (r2 >> 16)) d = (int16_t)r2;
    if (lane >= (r3 >> 16)) d = (int16_t)r3;
    j = lane + d;
    mine = lane < (field & 127);
}

// The sweep of one step for all cars of the workgroup, by every wave, in GROUPS of 64 consecutive rays of one car: a wave draws the
// next task (one LDS atomic), sets its 64 rays up, marches them until all have finished (march_all), stores the 64 ranges, and draws
// again.  Nothing is handed out ray by ray: no ranks, no per-lane bookkeeping, no partial refills -- the price is that a group
// lasts as long as its slowest ray (lane utilisation 0.61 against 0.78 with batched refills, tools/sweep_model.cpp), paid in lanes
// that sit masked out, not in instructions: a set-up costs about 60 instructions per 64 rays against 150 per 52, an iteration 24
// against 35.  Rays of a group are neighbours: they share field lines, and their ranges leave as one 256-byte row segment.
// With the rangefinders' own fan -- ray j + n/2 points exactly opposite to ray j (ftgp_create builds the table that way) -- a task is
// a PAIR of groups, j0 .. j0 + 63 and the same rays turned round: the second group keeps the first one's |direction|, reciprocals and
// slope slice (the two divisions and the sector search are half of a set-up) and only places its rays anew (ftgp_ray_place with
// sector ^ 3).  Tasks are drawn long-first across the workgroup's cars (group_order), so that the waves end a sweep together.
template <bool MULTI, bool WINDOW>
__device__ __forceinline__ void lidar_groups(const DeviceParams& P, ScalarParams G, const Lds& L, const LidarFrame* frames, const PairCull* pairs, const unsigned char* mmask,
                                             float* scan_rows, int* pool, int ncars_here, int ci0, bool scan_lds, bool second_half STAMP_ARG)
{
    typedef __attribute__((address_space(1))) float* global_f32;
    typedef __attribute__((address_space(1))) unsigned char* global_u8w;
    struct alignas(16) Task { int32_t x, y, z, w; };
    typedef const __attribute__((address_space(4))) Task* ScalarTasks;
    // WINDOW (implies scan_lds): a step whose ranges only the next step's drivers read -- every step of such a launch but its last.  The
    // draws come from the third table (plan_window_table): the rays outside the drivers' window are not marched, and no range goes to HBM --
    // the launch's last step writes every row.  An instantiation of its own, with a shell of its own for the table's plain draws (run_task below);
    // with WINDOW = false there is the masked body alone, the full sweep as it was.
    constexpr bool window_only = WINDOW;
    const int full_tasks = G->cars_per_block * G->tasks_per_car;
    const int R = G->n_rays, half = R >> 1, ntasks = window_only ? G->cars_per_block * G->win_tasks_per_car : full_tasks;
    const int W = G->width, H = G->height, fstride = G->fstride;
    const uint32_t plane256 = G->plane256;
    const int eighth = G->eighth, win_floats = G->win_floats;
    const float isx = G->inv_px_x_f, isy = G->inv_px_y_f, thr = 0.5f - G->snap_eps, nsf = G->slice_factor;
    const float r0 = sgpr(L.veh->ring_radius_f);
    const void* field = G->field;
    const ScalarTasks tasks = (ScalarTasks)G->task_tab + (window_only ? 2 * full_tasks : scan_lds ? 0 : full_tasks);      // (the second table: no ray goes to a scan window)
    const global_u8w ranges = (global_u8w)((global_f32)G->ranges + (size_t)ci0 * G->ranges_stride);      // the workgroup's first row
    const int mmask_stride = G->mmask_stride;
    const int lane = lane_here();
    // every ray of this sweep starts on the image (frame_write): no test per ray.  (The window-only sweep tests the word itself, behind opaque() at
    // each use: a bool hoisted out of the loop is kept as a lane mask and rebuilt with two vector instructions per set-up.)
    const int unsafe = sgpr(pool[4]);
    const bool all_safe = unsafe == 0;
    sweep_priority(second_half);
    for (;;) {                   // (ends: every draw moves the counter on)
        STAMP(ta);
        // (a task is drawn when the wave is ready for it, not earlier: drawing the next one before the march -- to hide the LDS round
        // trip -- reserves work behind a wave that may be on a long group, and cost 6 % on the headline and 12 % on config 2; drawing it
        // between the last march and its delivery is within noise: profiles/round5/ab_setup_latency_experiments.log)
        int g = 0;
        if (lane == 0) g = atomicAdd(pool, 1);
        g = __builtin_amdgcn_readfirstlane(g);
        if (g >= ntasks) break;
        // Draw g = the (g / cars_per_block)-th most expensive task (rays along the car's axis march longest, see group_order) of car slot
        // g % cars_per_block: the long tasks of every car go first, so that the waves of a workgroup end a sweep within a short group of each
        // other.  Everything about the draw that ftgp_create can know -- first ray, kind, car slot, where the car's LiDAR frame, its row of
        // ranges and its scan window start, whether the group's rays lie in the drivers' window -- comes as ONE 16-byte scalar load
        // (ftgp_task_entry; round 5: a division by multiplication, a table read and three 32- and 64-bit address products per group used to
        // stand here and in the delivery: a third of the kernel's scalar instructions).  The byte offset is formed in 32 bits -- a table is far
        // below 4 GB --, so it goes into the scalar load as it is: no 64-bit shift and add; and the four words are read as one vector, so that
        // they stay one load (field by field the compiler splits them and forms the address a second time).
        typedef int32_t TaskWords __attribute__((ext_vector_type(4)));
        Task task; { const TaskWords t = *(const __attribute__((address_space(4))) TaskWords*)((const __attribute__((address_space(4))) unsigned char*)tasks + ((uint32_t)g << 4)); task.x = t.x; task.y = t.y; task.z = t.z; task.w = t.w; }
        const int j0 = task.x & 0x3fff, kind = (task.x >> 14) & 3, c = (task.x >> 16) & 15;     // kind 0: one group; 1: a group and its opposite; 2: both halves in one group
        if (WINDOW && c >= ncars_here) continue;     // (a ragged last workgroup draws tasks of cars it does not have; the counter has moved)
        // The lanes of a draw that may be short of rays (every draw of the first two tables; of the window-only table the gathers, and all of it
        // where it is the first table again): which ray a lane marches, and whether it has one.
        auto masked_lanes = [&](int& j, bool& mine) __attribute__((always_inline)) {
            if (WINDOW && kind == 3) { asm volatile(""); gather_lanes(tasks + ntasks, j0, lane, j, mine); }      // window-only table: a gather, lanes from runs
            else if (kind == 2) { j = j0 + (lane & 31) + (lane >= 32 ? half : 0); mine = (lane & 31) < half - j0; }
            else { j = j0 + lane; mine = j < (kind == 1 ? half : R); }
            if (!WINDOW) mine = mine && c < ncars_here;               // (a ragged last workgroup draws tasks of cars it does not have)
        };
        // One task: set-up, march and delivery of its group, and of the opposite group where it has one.  MASKED = false: a PLAIN draw of the
        // window-only table (FTGP_TASK_MASKED clear: kind 0 or 1, 64 live rays a group, all of them in the drivers' window, no ray 0) -- lane l
        // marches ray j0 + l, there is no lane predicate and no exec region but march_all's own, and the delivery is one LDS store.
        auto run_task = [&](auto masked_tag, int j, bool lanes) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const bool mine = MASKED ? lanes : true;
        const LidarFrame* frame = reinterpret_cast<const LidarFrame*>(reinterpret_cast<const unsigned char*>(frames) + (task.y & 0xffff));
        FtgpRay ray;
        float du, dv, dxw, dyw, opu, opv;              // opu, opv: the ray's origin in pixels
        uint32_t sector;
        asm volatile("" : "=v"(du), "=v"(dv), "=v"(dxw), "=v"(dyw), "=v"(opu), "=v"(opv), "=v"(sector));      // (lanes that hold no ray never look at these: no moves to define them)
        // march the lanes' rays and deliver their ranges: ftgp_ray_range(), the inter-vehicle test, the stores
        auto finish = [&](bool active, int pass) {
            if (!active) return;
            uint32_t w;
            STAMP(tb);
            march_all(ray.s, w, opu, opv, ray.ivx, ray.ivy, du, dv, ray.base, ray.ax, ray.ay, thr, field);
            STAMP(tc); STAMP_ADD(10, tc - tb); STAMP_ADD(9, 1);
            float r = (w == 0u) ? fabsf(ray.s) : ray.result;
            if (MULTI && FTGP_DIAG_RUN_MATES) {
                // Rays also see the other cars of the env (a9).  One record per env-mate (PairCull, written with the frames) rules a
                // mate out with a dot product: it can only be touched if it lies in front of the ray and within `cull` of its line.
                const PairCull* mates = pairs + c * FTGP_PAIR_STRIDE;
                const int slot0 = sgpr(frame->slot0);
                // ... and one byte per (car, group) says which mates the group's rays can see at all (mate_masks): mostly none
                // (kidx: the task's rank in the list this sweep draws from -- the masks were computed for that list)
                const int kidx = task.y >> 16;
                uint32_t mm = (uint32_t)sgpr((int)mmask[c * mmask_stride + 2 * kidx + pass]);
                while (mm) {
                    const int k = __builtin_ctz(mm); mm &= mm - 1u;
                    const float4 q = *reinterpret_cast<const float4*>(mates + k);
                    const float al = fmaf(q.x, dxw, q.y * dyw);
                    if (al >= q.z) {
                        const float cull = L.veh->cull_radius;
                        if (r >= 0.0f && (al + r0) - cull > r) continue;             // the mate lies beyond the wall hit
                        const float rc = ray_vs_car(L.veh, frames + slot0 + k, q.x, q.y, dxw, dyw);
                        if (rc < INFINITY && (r < 0.0f || rc < r)) r = rc;
                    }
                }
            }
            // every range leaves for HBM now, 64 consecutive floats per wave (one 256-byte row segment); the window the on-device drivers
            // read next step -- ranges[0] and ranges[eighth : n - eighth] -- is kept in LDS as well.  (Not on a window-only step: nobody reads
            // its rows before the launch's last step has written them again.)
            const uint32_t j4 = (uint32_t)j << 2;
            if (!MASKED) { *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(scan_rows) + task.w + j4) = r; return; }      // (window class 1, no ray 0: see task.w below)
            if (!window_only) *(global_f32)(ranges + (j4 + (uint32_t)task.z)) = r;
            // task.w: byte offset of the car's scan row + ((eighth & 3) - eighth) floats, so that sample j sits at task.w + 4 j.  Whether the
            // group's rays lie inside the window, outside it or across one of its ends is the task's to know (two bits per pass; all zero in
            // the table of a launch whose drivers do not read the scan).  The rare cases sit behind scalar branches that the optimiser is kept
            // from turning into selects.
            const int wclass = (task.x >> (20 + 2 * pass)) & 3;
            if (wclass) {                        // (a group across an end of the window sends its outside rays to a spare word: one store site, no masks)
                float* dst = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(scan_rows) + task.w + j4);
                if (wclass == 2) { asm volatile(""); dst = (unsigned)(j - eighth) < (unsigned)(R - 2 * eighth) ? dst : reinterpret_cast<float*>(pool + 6); }
                *dst = r;
            }
            if ((task.x & (1 << 24)) && pass == 0) {          // the group holds ray 0: ranges[0] (fast.py:135) sits in the last float of the row
                asm volatile("");
                if (j == 0) *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(scan_rows) + task.w + 4 * (win_floats - 1 - (eighth & 3) + eighth)) = r;
            }
        };
        if (mine) {
            const float4 f4 = *reinterpret_cast<const float4*>(frame);      // u0, v0, chf, shf (one address for the wave)
            const float2 bd = L.ray[j];
            dxw = fmaf(f4.z, bd.x, -(f4.w * bd.y));
            dyw = fmaf(f4.w, bd.x, f4.z * bd.y);
            du = dxw * isx;
            dv = -(dyw * isy);
            const float pu = fmaf(du, -r0, f4.x);
            const float pv = fmaf(dv, -r0, f4.y);
            opu = pu; opv = pv;
            float ivx, ivy;
            rcp_abs2<true>(du, dv, ivx, ivy);
            ray.result = -1.0f;
            sector = ftgp_ray_sector(du, dv, ivx, ivy, nsf);
            ftgp_ray_place(ray, pu, pv, du, dv, ivx, ivy, sector, W, H, fstride, plane256, true, &P.sector_tab[0][0]);
            if (WINDOW ? opaque(unsafe) != 0 : !all_safe) {             // wave-uniform, rare: some car of the workgroup is near the image edge, off it, or has finished
                ftgp_ray_park_if_outside(ray, pu, pv, W, H);
                // a finished car's rangefinders are switched off (custom.py:1436-1439): its frame carries u0 = -inf, so the ray is
                // parked like any ray that starts off the image, and reads 0 instead of -1
                ray.result = (f4.x == -INFINITY) ? 0.0f : -1.0f;
            }
        }
        STAMP(td); STAMP_ADD(8, td - ta);
        finish(mine, 0);
        if (MASKED ? kind == 1 : (task.x & (1 << 14)) != 0) {                 // the same rays turned round: ray j + n/2 = -(ray j), exactly  (a plain draw is of kind 0 or 1)
            if (mine) {
                j += half;
                const float2 f2 = *reinterpret_cast<const float2*>(frame);
                du = -du; dv = -dv; dxw = -dxw; dyw = -dyw;
                const float pu = fmaf(du, -r0, f2.x);
                const float pv = fmaf(dv, -r0, f2.y);
                opu = pu; opv = pv;
                ftgp_ray_place(ray, pu, pv, du, dv, ray.ivx, ray.ivy, sector ^ 3u, W, H, fstride, plane256, true, &P.sector_tab[0][0]);
                if (WINDOW ? opaque(unsafe) != 0 : !all_safe) {
                    ftgp_ray_park_if_outside(ray, pu, pv, W, H);
                    ray.result = (f2.x == -INFINITY) ? 0.0f : -1.0f;
                }
            }
            finish(mine, 1);
        }
        };
        if (WINDOW && !(task.x & FTGP_TASK_MASKED)) run_task(std::false_type(), j0 + lane, true);
        else {
            if (WINDOW) asm volatile("");        // (a scalar branch, not selects)
            int j; bool mine;
            masked_lanes(j, mine);
            run_task(std::true_type(), j, mine);
        }
    }
}

// K2 in FTGP_LIDAR_FAKELIDAR mode: the reference's own 2-D LiDAR inside the step loop (option use_simulated_simulation_lidar,
// custom.py:987,1381-1393).  Per ray, in binary64 and in the order of the Python statements:
//   origin   i_x = (x / s) * W, i_y = -(y / s) * H of the car's position, s = 20 * scale (custom.py:1382-1384)
//   ray j    image-frame direction (dxw, -dyw), (dxw, dyw) = R(yaw) * fan[j]: the rangefinders' order
//   march    raycast.py:9-20: while dt[int(y), int(x)] > 2 and 0 <= x <= W and 0 <= y <= H: advance by dt
//   range    (distance / W) * s (custom.py:1392-1393), stored as binary32
// int() truncates toward zero and a negative index wraps like numpy's; an index past the end -- the reference's IndexError --
// ends the ray with range -1.
//
// march_fake(): the loop of raycast.py:12-17 for the 64 rays of a wave, hand-written like march_all() -- a ray leaves the loop by dropping
// out of exec -- with the statement order kept and the tests reduced to what can differ:
//   * numpy raises IndexError before the loop condition is looked at: an index is valid iff -n <= int(v) < n, i.e. (unsigned)(int(v) + n) < 2 n
//     (`bad`: the ray reads -1);
//   * a ray with x < 0 or y < 0 ends (its look-up, valid or wrapped, no longer matters: no load is issued for it); x <= W and y <= H need no
//     test of their own: a ray that is still here has int(x) < W, int(y) < H;
//   * what is left has 0 <= int(x) < W, 0 <= int(y) < H: one 24-bit multiply-add for the index, one 8-byte load (the table is
//     L2-resident: hit rate 0.998, profiles/round5/fakelidar_r5base.log), `nearest > 2` by v_cmpx.
// Binary64 throughout, one rounding per written operation (x += dx * nearest is a product and a sum).  `guard`: iterations after which a ray
// is given up with what it has accumulated (a caller's fan may hold a zero direction: the reference would loop for ever).
__device__ __forceinline__ void march_fake(double& x, double& y, double& dist, int& bad, double dx, double dy, int W, int H, const double* dt)
{
    double n = 0.0, t, u;
    int xi, yi, a, b;
    uint64_t sq, ex0;
    int guard = 1 << 16;
    // The look-up of an iteration is ISSUED before its tests are made (round 5, like march_all's): on an index clamped to the table -- for a ray
    // that passes the tests the clamp changes nothing, for one that fails them the answer is never looked at -- so that the dependent chain from
    // one look-up to the next is convert, clamp, index, load instead of convert and a dozen tests first; the tests run in the load's shadow.
    asm volatile(
        "s_mov_b64 %[ex0], exec\n"
        "L_fake_loop_%=:\n\t"
        "v_cvt_i32_f64_e32 %[xi], %[x]\n\t"                              // int(x): truncation toward zero
        "v_cvt_i32_f64_e32 %[yi], %[y]\n\t"
        "v_med3_i32 %[a], %[xi], 0, %[Wm1]\n\t"
        "v_med3_i32 %[b], %[yi], 0, %[Hm1]\n\t"
        "v_mad_u32_u24 %[a], %[b], %[W], %[a]\n\t"
        "v_lshlrev_b32_e32 %[a], 3, %[a]\n\t"
        "global_load_dwordx2 %[n], %[a], %[dt]\n\t"
        "v_add_u32_e32 %[a], %[W], %[xi]\n\t"
        "v_add_u32_e32 %[b], %[H], %[yi]\n\t"
        "v_cmp_le_u32_e32 vcc, %[W2], %[a]\n\t"                          // IndexError: not (-W <= int(x) < W) ...
        "v_cmp_le_u32_e64 %[sq], %[H2], %[b]\n\t"                        // ... or not (-H <= int(y) < H)
        "s_or_b64 vcc, vcc, %[sq]\n\t"
        "v_cndmask_b32_e64 %[bad], %[bad], -1, vcc\n\t"
        "v_cmp_gt_f64_e64 %[sq], 0, %[x]\n\t"                            // 0 <= x fails
        "s_or_b64 vcc, vcc, %[sq]\n\t"
        "v_cmp_gt_f64_e64 %[sq], 0, %[y]\n\t"
        "s_or_b64 vcc, vcc, %[sq]\n\t"
        "s_andn2_b64 exec, exec, vcc\n\t"                                // those rays are done
        "s_cbranch_execz L_fake_done_%=\n\t"
        "s_sub_u32 %[guard], %[guard], 1\n\t"
        "s_cbranch_scc1 L_fake_done_%=\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "v_cmpx_lt_f64_e32 vcc, 2.0, %[n]\n\t"                           // while nearest > eps
        "s_cbranch_execz L_fake_done_%=\n\t"
        "v_mul_f64 %[t], %[dx], %[n]\n\t"
        "v_mul_f64 %[u], %[dy], %[n]\n\t"
        "v_add_f64 %[x], %[x], %[t]\n\t"                                 // x += dx * nearest
        "v_add_f64 %[y], %[y], %[u]\n\t"                                 // y += dy * nearest
        "v_add_f64 %[dist], %[dist], %[n]\n\t"                           // distance += nearest
        "s_branch L_fake_loop_%=\n"
        "L_fake_done_%=:\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_mov_b64 exec, %[ex0]"
        : [x] "+v"(x), [y] "+v"(y), [dist] "+v"(dist), [bad] "+v"(bad), [n] "+v"(n), [t] "=&v"(t), [u] "=&v"(u), [xi] "=&v"(xi), [yi] "=&v"(yi), [a] "=&v"(a), [b] "=&v"(b),
          [sq] "=&s"(sq), [ex0] "=&s"(ex0), [guard] "+s"(guard)
        : [dx] "v"(dx), [dy] "v"(dy), [W] "s"(W), [H] "s"(H), [W2] "s"(2 * W), [H2] "s"(2 * H), [Wm1] "s"(W - 1), [Hm1] "s"(H - 1), [dt] "s"(dt)
        : "vcc", "scc", "memory");
}

// The FAKELIDAR sweep of one step for all cars of the workgroup: the task list, the draw and the delivery of lidar_groups() -- groups of 64
// neighbouring rays of one car, long-first across the workgroup's cars, a pair's two groups one after the other -- around march_fake().
// What depends on the car alone -- i_x, i_y (two binary64 divisions) and the heading -- comes with its LiDAR frame (frame_write).
__device__ __forceinline__ void lidar_fake(ScalarParams G, const LidarFrame* frames, float* scan_rows, int* pool, int ncars_here, int ci0, bool scan_lds, bool window_only)
{
    typedef __attribute__((address_space(1))) float* global_f32;
    typedef __attribute__((address_space(1))) unsigned char* global_u8w;
    struct alignas(16) Task { int32_t x, y, z, w; };             // DeviceParams::task_tab (see lidar_groups)
    typedef const __attribute__((address_space(4))) Task* ScalarTasks;
    const int full_tasks = G->cars_per_block * G->tasks_per_car;       // window_only: as in lidar_groups -- the third table, no unread ray marched, no range to HBM
    const int R = G->n_rays, half = R >> 1, ntasks = window_only ? G->cars_per_block * G->win_tasks_per_car : full_tasks;
    const int W = G->width, H = G->height;
    const int eighth = G->eighth, win_floats = G->win_floats;
    const double s = G->map_size;
    const double* dt = G->edt;
    const double* __restrict__ fan = G->fan_dirs;
    const ScalarTasks tasks = (ScalarTasks)G->task_tab + (window_only ? 2 * full_tasks : scan_lds ? 0 : full_tasks);
    const global_u8w ranges = (global_u8w)((global_f32)G->ranges + (size_t)ci0 * G->ranges_stride);
    const int lane = lane_here();
    for (;;) {
        int g = 0;
        if (lane == 0) g = atomicAdd(pool, 1);
        g = __builtin_amdgcn_readfirstlane(g);
        if (g >= ntasks) break;
        Task task; { const uint32_t gu = (uint32_t)g; task.x = tasks[gu].x; task.y = tasks[gu].y; task.z = tasks[gu].z; task.w = tasks[gu].w; }
        const int j0 = task.x & 0x3fff, kind = (task.x >> 14) & 3, c = (task.x >> 16) & 15;
        int j; bool mine;
        if (kind == 3) gather_lanes(tasks + ntasks, j0, lane, j, mine);      // (the window-only table alone has gathers)
        else if (kind == 2) { j = j0 + (lane & 31) + (lane >= 32 ? half : 0); mine = (lane & 31) < half - j0; }
        else { j = j0 + lane; mine = j < (kind == 1 ? half : R); }
        mine = mine && c < ncars_here;
        const LidarFrame* f = reinterpret_cast<const LidarFrame*>(reinterpret_cast<const unsigned char*>(frames) + (task.y & 0xffff));
        for (int pass = 0; pass < (kind == 1 ? 2 : 1); ++pass, j += half) {
            if (!mine) continue;
            float r = 0.0f;                                       // a finished car's rangefinders are switched off (custom.py:1436-1439): its scan reads 0
            if (!f->finished) {
                const double ch = f->x, sh = f->y;                // FAKELIDAR frames: heading (cos, sin) in binary64 (frame_write)
                const double bx = fan[2 * j], by = fan[2 * j + 1];
                const double dxw = ch * bx - sh * by, dyw = sh * bx + ch * by;
                double x = f->lcx, y = f->lcy, distance = 0.0;    // FAKELIDAR frames: i_x, i_y (custom.py:1383-1384)
                int bad = 0;
                march_fake(x, y, distance, bad, dxw, -dyw, W, H, dt);      // image rows grow downwards
                r = bad ? -1.0f : (float)((distance / (double)W) * s);     // ranges /= original_width; ranges *= s (custom.py:1392-1393)
            }
            const uint32_t j4 = (uint32_t)j << 2;
            if (!window_only) *(global_f32)(ranges + (j4 + (uint32_t)task.z)) = r;
            const int wclass = (task.x >> (20 + 2 * pass)) & 3;   // the delivery of lidar_groups(): window classes from the task
            if (wclass) {
                float* dst = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(scan_rows) + task.w + j4);
                if (wclass == 2) { asm volatile(""); dst = (unsigned)(j - eighth) < (unsigned)(R - 2 * eighth) ? dst : reinterpret_cast<float*>(pool + 6); }
                *dst = r;
            }
            if ((task.x & (1 << 24)) && pass == 0) {
                asm volatile("");
                if (j == 0) *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(scan_rows) + task.w + 4 * (win_floats - 1 - (eighth & 3) + eighth)) = r;
            }
        }
    }
}

// device arithmetic the kernels rely on, checked over every binary32 bit pattern: rcp_abs2() == |1 / x| (IEEE division) in either slot
__global__ void ftgp_selftest_rcp_kernel(unsigned long long* __restrict__ mismatches)
{
    unsigned long long bad = 0;
    const uint32_t per = 1u << 12;                                     // 2^20 threads x 2^12 patterns
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t k = 0; k < per; ++k) {
        const float x = __uint_as_float(t * per + k);
        float a, a2;
        rcp_abs2(x, 3.0f, a, a2);
        const float b = fabsf(1.0f / x);
        float c, c2;
        rcp_abs2(0.7f, x, c2, c);                              // second operand too (and the first in range: the slow path only if x needs it)
        const bool same = (__float_as_uint(a) == __float_as_uint(b) || (a != a && b != b)) && (__float_as_uint(c) == __float_as_uint(b) || (c != c && b != b));
        bad += same ? 0 : 1;
    }
    if (bad) atomicAdd(mismatches, bad);
}

// =============================================================================================
// K3: lap progress (custom.py:1340-1372)
// =============================================================================================
// (start and finish_step -- 64 bits each, touched on line crossings only -- stay in the car's record and are reached through `steps64`:
// carried in registers they would push the K1 + K3 wave over the kernel's 64-register budget)
struct Race { int32_t completion, laps, offset, good_start, finished, off_track, delta, n_times; double dist2; };

__device__ __forceinline__ void progress_update(const DeviceParams& P, Race& s, int64_t steps, int closest, double best, double* __restrict__ times, int64_t* steps64 /* &start, &finish_step */)
{
    s.dist2 = best;                                       // custom.py:1343 (squared)
    s.off_track = best > 1.0;                             // custom.py:1344
    if (s.off_track) return;                              // custom.py:1345: progress frozen off-track
    const int completion = ((closest - s.offset) % 100 + 100) % 100;
    const int delta = completion - s.completion;
    s.delta = (((completion - s.completion + 50) % 100) + 100) % 100 - 50;
    if (abs(delta) > 90) {
        // one store site for the ring (an appended lap time, or the mark of an emptied slot): two would not fit the K1 + K3 wave's registers
        double val = (double)(steps - steps64[0]) * P.dt;      // lap_time
        int slot = -1;
        if (s.delta < 0) {                                // backwards across the line, custom.py:1352-1356
            s.laps -= 1;
            s.good_start = 0;
            if (s.n_times != 0) {                             // times.pop()
                // the ring keeps the newest FTGP_MAX_LAP_TIMES: beyond that the popped entry sits in the slot of the oldest one the list would
                // still show (it was overwritten when the popped lap was appended) -- that slot is marked empty (NaN: skipped by every reader)
                if (s.n_times > FTGP_MAX_LAP_TIMES) { slot = s.n_times - 1; val = val * __builtin_nan(""); }
                s.n_times -= 1;
            }
        } else if (s.delta > 0) {                         // custom.py:1357-1366
            if (s.good_start) {
                slot = s.n_times;                             // times.append(lap_time): a ring of the newest FTGP_MAX_LAP_TIMES
                s.n_times += 1;
                steps64[0] = steps;
            }
            s.laps += 1;
            s.good_start = 1;
        }
        if (slot >= 0) times[slot & (FTGP_MAX_LAP_TIMES - 1)] = val;
    }
    if (s.laps >= P.lap_target) {                         // custom.py:1367-1370; the step of the first time orders the winners (custom.py:1368-1369)
        if (!s.finished) steps64[1] = steps;
        s.finished = 1;
    }
    s.completion = completion;
}

__device__ __forceinline__ void race_load(Race& r, const CarCore* st)
{
    r.completion = st->completion; r.laps = st->laps; r.offset = st->offset;
    r.good_start = st->good_start; r.finished = st->finished; r.off_track = st->off_track; r.delta = st->delta;
    r.n_times = st->n_times; r.dist2 = st->dist2;
}
__device__ __forceinline__ void race_store(const Race& r, CarCore* st)
{
    st->completion = r.completion; st->laps = r.laps;
    st->good_start = r.good_start; st->finished = r.finished; st->off_track = r.off_track; st->delta = r.delta;
    st->n_times = r.n_times; st->dist2 = r.dist2;
}

// =============================================================================================
// K1: integrate one dt (reduced planar model of template/mushr.em.xml stepped by mj_step, custom.py:1425)
// =============================================================================================

// 32 wall bits of bitmap row `row` starting at column x0 (bit i = column x0 + i; columns outside the image read 0)
__device__ __forceinline__ uint32_t wall_window(const uint32_t* __restrict__ row, int wpr, int x0)
{
    const int wi = x0 >> 5, sh = x0 & 31;
    const uint32_t lo = (wi >= 0 && wi < wpr) ? row[wi] : 0u;
    const uint32_t hi = (wi + 1 >= 0 && wi + 1 < wpr) ? row[wi + 1] : 0u;
    return sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
}

// One circle (centre (px, py), radius r) against the wall pixels, in two parts so that neither keeps the other's values in
// registers (the kernel runs under a 64-VGPR budget): the search returns the pixel of deepest penetration -- ties go to the
// first pixel in raster order -- and the force part turns it into the penalty spring/damper term along the contact normal.
struct WallHit { double pen; int cx, cy; bool found; };

__device__ __forceinline__ WallHit wall_search(const DeviceParams& P, const uint32_t* __restrict__ bits, const uint32_t* __restrict__ nearbits,
                                               double px, double py, double r)
{
    WallHit h; h.pen = 0.0; h.cx = 0; h.cy = 0; h.found = false;
    const int W = P.width, H = P.height, wpr = P.words_per_row;
    const double sx = P.px_size_x, sy = P.px_size_y;
    const int nx = (int)ceil(r * P.inv_px_x), ny = (int)ceil(r * P.inv_px_y);
    const double u = (px - P.origin_x) * P.inv_px_x, w = (P.origin_y - py) * P.inv_px_y;
    const int ix = (int)floor(u), iy = (int)floor(w);
    if (ix < 0 || ix >= W || iy < 0 || iy >= H) return h;
    if (!((nearbits[(size_t)iy * wpr + (ix >> 5)] >> (ix & 31)) & 1u)) return h;      // no wall pixel within the window
    const int wx = 2 * nx + 1;
    for (int dy = -ny; dy <= ny; ++dy) {
        const int cy = iy + dy;
        if (cy < 0 || cy >= H) continue;
        const uint32_t* row = bits + (size_t)cy * wpr;
        for (int cb = 0; cb < wx; cb += 32) {
            const int x0 = ix - nx + cb, nb = wx - cb < 32 ? wx - cb : 32;
            uint32_t win = wall_window(row, wpr, x0);
            if (nb < 32) win &= (1u << nb) - 1u;
            while (win) {
                const int cx = x0 + __builtin_ctz(win);
                win &= win - 1u;
                const double x0w = P.origin_x + (double)cx * sx, x1w = x0w + sx;
                const double y1w = P.origin_y - (double)cy * sy, y0w = y1w - sy;
                const double qx = px < x0w ? x0w : (px > x1w ? x1w : px);
                const double qy = py < y0w ? y0w : (py > y1w ? y1w : py);
                const double ex = px - qx, ey = py - qy;
                const double d2 = ex * ex + ey * ey;
                if (d2 >= r * r) continue;
                const double pen = r - sqrt(d2);
                if (!h.found || pen > h.pen) { h.pen = pen; h.cx = cx; h.cy = cy; h.found = true; }
            }
        }
    }
    return h;
}

__device__ __forceinline__ Force wall_force(const DeviceParams& P, const WallHit& h, double px, double py, double vx, double vy, double wz,
                                            double rxw, double ryw, double stiffness, double damping)
{
    Force out = { 0.0, 0.0, 0.0 };
    const double sx = P.px_size_x, sy = P.px_size_y;
    const double x0w = P.origin_x + (double)h.cx * sx, x1w = x0w + sx;
    const double y1w = P.origin_y - (double)h.cy * sy, y0w = y1w - sy;
    const double qx = px < x0w ? x0w : (px > x1w ? x1w : px);
    const double qy = py < y0w ? y0w : (py > y1w ? y1w : py);
    const double ex = px - qx, ey = py - qy;
    const double d = sqrt(ex * ex + ey * ey);
    double nxv, nyv;
    if (d > 0.0) { nxv = ex / d; nyv = ey / d; }
    else {
        const double mx = px - (x0w + 0.5 * sx), my = py - (y0w + 0.5 * sy);
        const double mm = sqrt(mx * mx + my * my);
        if (mm > 0.0) { nxv = mx / mm; nyv = my / mm; } else { nxv = 0.0; nyv = 0.0; }
    }
    const double vcx = vx - wz * ryw, vcy = vy + wz * rxw;
    const double vn = vcx * nxv + vcy * nyv;
    const double mag = stiffness * h.pen - damping * vn;
    if (mag <= 0.0) return out;
    out.fx = mag * nxv; out.fy = mag * nyv; out.tz = rxw * out.fy - ryw * out.fx;
    return out;
}

// everything a later block needs is re-read from LDS after this point instead of being carried in registers
#define FTGP_FORGET_REGISTERS() asm volatile("" ::: "memory")

// chassis circle k (body (contact_x[k], 0)) or wheel softener k (body (wheel_x[k], wheel_y[k])) of car `st` against the walls
__device__ __forceinline__ Force wall_term(const DeviceParams& P, const FtgpVehicle& v, const CarCore* st, int k, bool softener)
{
    WallHit h; double px, py;
    {
        const double qw = st->qw, qz = st->qz;
        const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
        const double rxw = softener ? ch * v.wheel_x[k] - sh * v.wheel_y[k] : ch * v.contact_x[k];
        const double ryw = softener ? sh * v.wheel_x[k] + ch * v.wheel_y[k] : sh * v.contact_x[k];
        px = st->x + rxw; py = st->y + ryw;
        // (the two bitmap pointers are wave-uniform: in scalar registers they do not count against the 64 vector registers)
        h = wall_search(P, uniform_ptr(P.bits), uniform_ptr(P.nearbits), px, py, softener ? v.softener_radius : v.contact_radius);
    }
    FTGP_FORGET_REGISTERS();
    Force t = { 0.0, 0.0, 0.0 };
    if (h.found) {
        const double qw = st->qw, qz = st->qz;
        const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
        const double rxw = softener ? ch * v.wheel_x[k] - sh * v.wheel_y[k] : ch * v.contact_x[k];
        const double ryw = softener ? sh * v.wheel_x[k] + ch * v.wheel_y[k] : sh * v.contact_x[k];
        t = wall_force(P, h, px, py, st->vx, st->vy, st->wz, rxw, ryw, v.contact_stiffness, v.contact_damping);
    }
    return t;
}

// Circles of this car against the circles of ONE other car of the env (penalty spring/damper, pre-step states): the sum of the nine
// circle pairs' forces, from +0, in the order i, j -- the specification adds the contacts with each env-mate up on their own and lets the
// mates' sums join the car's force in the order of the mates (round 5: that is what lets a car's four lanes take a mate each; rounds 1-4
// ran one sum over k, i, j on one lane, 27 dependent rounds of this loop body on the step's critical path).  The loop stays rolled and every
// operand is re-read from LDS where it is used, so that the only values carried around it are the running sum and a few indices.
__device__ __forceinline__ Force car_contact_mate(const FtgpVehicle& v, const CarCore* me, const CarCore* b)
{
    Force f = { 0.0, 0.0, 0.0 };
    #pragma unroll 1
    for (int ij = 0; ij < 9; ++ij) {
        FTGP_FORGET_REGISTERS();
        const int i = ij / 3, j = ij - 3 * i;
        const double r2 = 2.0 * v.contact_radius;
        double rxw, ryw, sxw, syw, ex, ey;
        {
            const double qw = me->qw, qz = me->qz;
            const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
            rxw = ch * v.contact_x[i]; ryw = sh * v.contact_x[i];
            const double bqw = b->qw, bqz = b->qz;
            const double cb = 1.0 - 2.0 * (bqz * bqz), sb = 2.0 * (bqw * bqz);
            sxw = cb * v.contact_x[j]; syw = sb * v.contact_x[j];
            const double px = me->x + rxw, py = me->y + ryw;
            const double qx = b->x + sxw, qy = b->y + syw;
            ex = px - qx; ey = py - qy;
        }
        const double d2 = ex * ex + ey * ey;
        if (d2 >= r2 * r2 || d2 <= 0.0) continue;
        const double d = sqrt(d2);
        const double nxv = ex / d, nyv = ey / d;
        const double swz = me->wz, bwz = b->wz;
        const double vax = me->vx - swz * ryw, vay = me->vy + swz * rxw;
        const double vbx = b->vx - bwz * syw, vby = b->vy + bwz * sxw;
        const double vn = (vax - vbx) * nxv + (vay - vby) * nyv;
        const double mag = v.contact_stiffness * (r2 - d) - v.contact_damping * vn;
        if (mag <= 0.0) continue;
        const double fx = mag * nxv, fy = mag * nyv;
        f.fx += fx; f.fy += fy; f.tz += rxw * fy - ryw * fx;
    }
    return f;
}

// LiDAR frame of a car at its current pose (lidar_car() of the oracle: centre, heading, binary32 pixel coordinates).
// Returns whether every ray of this car is KNOWN to start on the image: the car races, and its LiDAR centre is finite and at
// least edge_margin (ring radius in pixels + 2) away from every image edge.  When that holds for all cars of the workgroup the
// sweep initialises its rays without the on-image test (ftgp_ray_init, assume_inside).
__device__ __forceinline__ bool frame_write(const DeviceParams& P, const FtgpVehicle& v, const CarCore* st, LidarFrame* fr, int slot)
{
    const double qw = st->qw, qz = st->qz;
    const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
    const double lcx = st->x + (ch * v.lidar_x - sh * v.lidar_y);
    const double lcy = st->y + (sh * v.lidar_x + ch * v.lidar_y);
    const int finished = st->finished;
    const float u0 = (float)((lcx - P.origin_x) * P.inv_px_x), v0 = (float)((P.origin_y - lcy) * P.inv_px_y);
    fr->u0 = finished ? -INFINITY : u0;                       // -inf: rangefinders switched off (see lidar_groups)
    fr->v0 = v0;
    fr->chf = (float)ch; fr->shf = (float)sh;
    fr->lcx = lcx; fr->lcy = lcy;
    fr->x = st->x; fr->y = st->y; fr->qw = qw; fr->qz = qz;
    if (sgpr(P.lidar_mode) == FTGP_LIDAR_FAKELIDAR) {          // what lidar_fake() needs of the car: i_x, i_y (custom.py:1382-1384) and the heading, binary64
        fr->lcx = (st->x / P.map_size) * (double)P.width; fr->lcy = -(st->y / P.map_size) * (double)P.height;
        fr->x = ch; fr->y = sh;
    }
    fr->finished = finished;
    if (sgpr(P.cars_per_env) > 1) {       // what the inter-vehicle cull reads (this function sits on the driver -> dynamics chain: nothing it does not need)
        fr->slot0 = slot - slot % P.cars_per_env;
        fr->fx = (float)st->x; fr->fy = (float)st->y;
    }
    const float m = P.edge_margin;
    return !finished && u0 >= m && u0 <= (float)P.width - m && v0 >= m && v0 <= (float)P.height - m;      // false for a NaN
}

// The env-mate records of car c for the frames just written (see PairCull): one lane per (car, mate) pair.
__device__ __forceinline__ void pair_cull_write(const LidarFrame* frames, PairCull* pairs, int c, int k, int cars_per_env, float cull, float r0)
{
    const LidarFrame* me = frames + c;
    const int mate = me->slot0 + k;
    PairCull p; p.bx = 0.0f; p.by = 0.0f; p.t = INFINITY; p.pad = 0.0f;
    if (k < cars_per_env && mate != c && !me->finished && !frames[mate].finished) {
        p.bx = (float)(frames[mate].x - me->lcx); p.by = (float)(frames[mate].y - me->lcy);
        const float d2 = p.bx * p.bx + p.by * p.by, close = 2.0f * cull + r0;
        p.t = d2 <= close * close ? -INFINITY : sqrtf(d2 - cull * cull) * 0.9999f;
    }
    pairs[c * FTGP_PAIR_STRIDE + k] = p;
}

// Multi-car envs: which env-mates can the rays of a GROUP see?  The sweep tests a ray against a mate only if the mate lies inside the
// ray's cone (PairCull); most groups of 64 neighbouring rays look nowhere near any mate, and finding that out ray by ray -- a record
// read, a dot product, a compare and a wave-wide vote per mate and group -- was a third of the multi-car sweep.  So it is decided once
// per (car, group, mate), lane-parallel, by the wave that has just written the frames: a ray of the group lies within 32 ray
// spacings (10.7 degrees at 1080 rays; the bound below is computed for the actual fan spacing) of the group's middle ray d_g, so it can
// only pass its own test  B . d >= t  if  B . d_g >= cos(gamma) t - sin(gamma) cull  (cos of a sum of angles), gamma = that half-width
// plus what the 0.9999 in t and binary32 rounding can add.  One byte per (car, group): bit k = env-mate k may be visible.  A mask that
// says "may" too often costs time, never a result: the exact tests follow.
typedef const __attribute__((address_space(4))) int32_t* ScalarInts;
__device__ __forceinline__ void mate_masks(const LidarFrame* frames, const PairCull* pairs, unsigned char* mmask, int mmask_stride, ScalarInts order,
                                           const float2* __restrict__ ray_tab, int R, int tasks, int cars_per_env, float cull, float cg, float sg,
                                           int ncars_here, int first, int step)
{
    const int slots = 2 * tasks;
    for (int idx = first; idx < ncars_here * slots; idx += step) {
        const int c = idx / slots, s = idx - c * slots;
        const int ent = order[s >> 1], j0 = ent & 0xffff, kind = ent >> 16;
        uint32_t m = 0;
        if (kind >= 2 || cg < -1.0f) m = (s & 1) ? 0u : 0xffu;                // both half-fans in one group, a gather (kind 3), or a fan the bound does not cover: look at every mate
        else if (!(s & 1) || kind == 1) {
            const int jc = min(j0 + 32, (kind == 1 ? (R >> 1) : R) - 1);
            const float2 bd = ray_tab[jc];
            const LidarFrame* me = frames + c;
            float dxw = fmaf(me->chf, bd.x, -(me->shf * bd.y)), dyw = fmaf(me->shf, bd.x, me->chf * bd.y);
            if (s & 1) { dxw = -dxw; dyw = -dyw; }                                   // the opposite group
            for (int k = 0; k < cars_per_env; ++k) {
                const float4 q = *reinterpret_cast<const float4*>(pairs + c * FTGP_PAIR_STRIDE + k);
                const float al = fmaf(q.x, dxw, q.y * dyw);
                if (al >= fmaf(cg, q.z, -(sg * cull)) - 1e-4f) m |= 1u << k;          // (t = +inf: never -- myself, a finished car; t = -inf: always)
            }
        }
        mmask[c * mmask_stride + s] = (unsigned char)m;
    }
}

// One exchange of K3's argmin inside a quad of lanes: every lane sees the (distance, index) of the lane QUAD_PERM names and keeps the better pair
template <int QUAD_PERM>
__device__ __forceinline__ void quad_argmin_step(double& best, int& idx)
{
    const int lo = __double2loint(best), hi = __double2hiint(best);
    const double ob = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, QUAD_PERM, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, QUAD_PERM, 0xf, 0xf, false));
    const int oi = __builtin_amdgcn_update_dpp(idx, idx, QUAD_PERM, 0xf, 0xf, false);
    if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
}

// K1 + K3 for every car of the workgroup by ONE wave, four lanes per car (lane = 4 * car + r).
//   K1  lane r evaluates wheel r (fl, fr, bl, br), then wall-contact circle r (r < 3), then wheel softener r (bubble_wrap);
//       the force terms go to an LDS staging row and lane 0 of the car adds them up in the specification's order
//       (wheels 0..3, circles 0..2, softeners 0..3 -- a term that touches nothing is +0 and changes nothing, because the
//       running sum starts at +0 and can never become -0), adds the car-car contacts and integrates.  All lanes read the
//       pre-step states before any lane commits, so multi-car envs need no staging buffer for the states.
//   K3  25 centre-line points per lane, first minimum wins; steps += 1 happens between K1 and K3, as in custom.py:1425-1426
//       followed by the head of the next loop iteration.
// Then the LiDAR frames of the next step are written.
// DYN: the table of per-car dynamics is on (ftgp_set_dynamics): the eight entries of the car's row and its wheel loads come from the car's
// own record in LDS (`dyn`, FTGP_DYN_RECORD doubles per car slot: the car's four lanes read one address), everything else from L.veh as ever.
template <bool MULTI, bool DYN>
__device__ __forceinline__ void dynamics_lanes(const DeviceParams& P, const Lds& L, LidarFrame* next_frames, PairCull* next_pairs, unsigned char* next_mmask, ScalarInts order, bool win_next,
                                               int* unsafe_next, int ncars_here, int ci0, const double* dyn)
{
    const int lane = lane_here();
    const int c = lane >> 2, r = lane & 3;
    const bool on = c < ncars_here;
    CarCore* st = L.cars + (on ? c : 0);
    Force* terms = L.terms + (on ? c : 0) * FTGP_FORCE_TERMS;
    const FtgpVehicle& v = L.veh->v;
    const bool finished = st->finished != 0;
    SUBSTAMP_BEGIN();
    {   // ---- wheel r
        const double* mine = dyn + (on ? c : 0) * FTGP_DYN_RECORD;      // (DYN only)
        const double qw = st->qw, qz = st->qz;
        const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
        const double vx = st->vx, vy = st->vy, wz = st->wz;
        // Ackermann coupling, mushr.em.xml:185-186: q + 0.375 q^2 + 0.140625 q^3 - 0.0722656 q^4 (fl), the odd signs flipped for fr
        const double q = st->qs;
        // (the odd coefficients by sign flips of the products: a negation is exact, and no 64-bit constant has to be selected per lane)
        const double c1 = (r == 0) ? 0.375 : -0.375;
        const double q4 = q * 0.0722656, t3 = (r == 0) ? -q4 : q4;
        const double steer = q * (1.0 + q * (c1 + q * (0.140625 + t3)));
        const bool tri = sgpr(v.kind) == FTGP_VEHICLE_TRICYCLE;         // legacy differential-drive car (car.em.xml): no steering, two driven wheels
        const double ang = (!tri && r < 2) ? steer : 0.0;               // wheels that do not steer: the polynomials give exactly (1, 0) at 0
        const double cwi = spec_cos(ang), swi = spec_sin(ang);
        double torque;
        if (!tri) {
            // velocity servo on the tendon = mean wheel spin, mushr.em.xml:180,191-196
            const double wbar = 0.25 * (((st->w[0] + st->w[1]) + st->w[2]) + st->w[3]);
            double fa;
            if constexpr (DYN) {
                const double flim = mine[kDynThrottleForceLimit];
                fa = mine[kDynThrottleKv] * (st->u_speed - v.throttle_gear * wbar);
                if (fa > flim) fa = flim;
                if (fa < -flim) fa = -flim;
            } else {
                fa = v.throttle_kv * (st->u_speed - v.throttle_gear * wbar);
                if (fa > v.throttle_force_limit) fa = v.throttle_force_limit;
                if (fa < -v.throttle_force_limit) fa = -v.throttle_force_limit;
            }
            torque = (v.throttle_gear * 0.25) * fa;
        } else {
            // two torque motors on the tendons 0.5 (l + r) and 0.5 (r - l), controls clamped to their ctrlrange (car.em.xml:126-139)
            double uf = st->u_speed, ut = st->u_steer;
            if (uf > v.motor_forward_limit) uf = v.motor_forward_limit;
            if (uf < -v.motor_forward_limit) uf = -v.motor_forward_limit;
            if (ut > v.motor_turn_limit) ut = v.motor_turn_limit;
            if (ut < -v.motor_turn_limit) ut = -v.motor_turn_limit;
            torque = (r == 0) ? 0.5 * uf - 0.5 * ut : 0.5 * uf + 0.5 * ut;
        }
        const bool rolling = !(tri && r >= 2);                          // the caster is frictionless and there is no fourth wheel
        const double wi = st->w[r];
        const double wx_ = v.wheel_x[r], wy_ = v.wheel_y[r];
        const double rxw = ch * wx_ - sh * wy_;
        const double ryw = sh * wx_ + ch * wy_;
        const double vpx = vx - wz * ryw, vpy = vy + wz * rxw;
        const double fdx = ch * cwi - sh * swi, fdy = sh * cwi + ch * swi;
        const double vlong = (vpx * fdx + vpy * fdy) - v.wheel_radius * wi;
        const double vlat = vpy * fdx - vpx * fdy;
        double flong, flat, lim;
        if constexpr (DYN) {
            flong = -(mine[kDynTireDamping] * vlong); flat = -(mine[kDynTireDamping] * vlat);
            lim = mine[kDynFriction] * mine[kDynWheelLoad + r];
        } else {
            flong = -(v.tire_damping * vlong); flat = -(v.tire_damping * vlat);
            lim = v.friction * L.veh->wheel_load[r];
        }
        const double m2 = flong * flong + flat * flat;
        if (m2 > lim * lim) { const double sc = lim / sqrt(m2); flong = flong * sc; flat = flat * sc; }
        Force t;
        t.fx = flong * fdx - flat * fdy; t.fy = flong * fdy + flat * fdx; t.tz = rxw * t.fy - ryw * t.fx;
        const double dt = P.dt;
        const double wn = (v.wheel_inertia * wi + dt * (torque - v.wheel_radius * flong)) / (v.wheel_inertia + dt * v.wheel_damping);
        if (!rolling) { t.fx = 0.0; t.fy = 0.0; t.tz = 0.0; }
        if (on) { terms[r] = t; L.wnew[(on ? c : 0) * 4 + r] = rolling ? wn : wi; }
    }
    FTGP_FORGET_REGISTERS();
    SUBSTAMP(0);
    {   // ---- wall-contact circle r and wheel softener r (a shadowed car collides with nothing, custom.py:1452-1457)
        Force t = { 0.0, 0.0, 0.0 };
        if (on && !finished && r < 3) t = wall_term(P, v, st, r, false);
        if (on && r < 3) terms[4 + r] = t;
        FTGP_FORGET_REGISTERS();
        Force u = { 0.0, 0.0, 0.0 };
        if (on && !finished && P.bubble_wrap) u = wall_term(P, v, st, r, true);        // custom.py:1041-1055, mushr.em.xml:65-67,126-129
        if (on) terms[7 + r] = u;
    }
    FTGP_FORGET_REGISTERS();
    SUBSTAMP(1);
    if (MULTI) {                     // ---- car-car contacts: lane r takes env-mates r and r + 4 (a shadowed car collides with nothing, custom.py:1452-1457)
        #pragma unroll 1
        for (int k = r; k < sgpr(P.cars_per_env); k += 4) {
            Force t = { 0.0, 0.0, 0.0 };
            const CarCore* b = st + (k - c % P.cars_per_env);          // env-mate k of this car's env (cars of an env are neighbours in the workgroup)
            if (on && !finished && b != st && !b->finished) t = car_contact_mate(v, st, b);
            if (on) L.mates[c * FTGP_PAIR_STRIDE + k] = t;
        }
        FTGP_FORGET_REGISTERS();
    }
    wave_lds_sync();                 // every lane has read the pre-step states; the force terms are staged
    SUBSTAMP(2);
    if (on && r == 0) {
        Force f = { 0.0, 0.0, 0.0 };
        #pragma unroll 1
        for (int k = 0; k < FTGP_FORCE_TERMS; ++k) { const Force t = terms[k]; f.fx += t.fx; f.fy += t.fy; f.tz += t.tz; }
        const double qw = st->qw, qz = st->qz;
        if (MULTI) {                 // the env-mates' contact sums, in the order of the mates (zeros where nothing touches)
            #pragma unroll 1
            for (int k = 0; k < P.cars_per_env; ++k) { const Force t = L.mates[c * FTGP_PAIR_STRIDE + k]; f.fx += t.fx; f.fy += t.fy; f.tz += t.tz; }
        }
        const double dt = P.dt;
        Dyn o;
        if constexpr (DYN) {         // (the car's own mass, yaw inertia and steering servo)
            const double* mine = dyn + c * FTGP_DYN_RECORD;
            o.vx = st->vx + dt * (f.fx / mine[kDynMass]);
            o.vy = st->vy + dt * (f.fy / mine[kDynMass]);
            o.wz = st->wz + dt * (f.tz / mine[kDynIzz]);
            o.qsd = (v.steer_inertia * st->qsd + dt * (mine[kDynSteerKp] * (st->u_steer - st->qs))) / (v.steer_inertia + dt * mine[kDynSteerDamping]);
        } else {
            o.vx = st->vx + dt * (f.fx / v.mass);
            o.vy = st->vy + dt * (f.fy / v.mass);
            o.wz = st->wz + dt * (f.tz / v.izz);
            // position servo on the steering joint, implicit damping (mushr.em.xml:78,179)
            o.qsd = (v.steer_inertia * st->qsd + dt * (v.steer_kp * (st->u_steer - st->qs))) / (v.steer_inertia + dt * v.steer_damping);
        }
        o.qs = st->qs + dt * o.qsd;
        if (o.qs > v.steer_limit) { o.qs = v.steer_limit; if (o.qsd > 0.0) o.qsd = 0.0; }
        if (o.qs < -v.steer_limit) { o.qs = -v.steer_limit; if (o.qsd < 0.0) o.qsd = 0.0; }
        if (v.kind == FTGP_VEHICLE_TRICYCLE) { o.qs = st->qs; o.qsd = st->qsd; }       // no steering joint
        // semi-implicit Euler: positions with the new velocities
        const double h = (0.5 * dt) * o.wz;
        const double chh = spec_cos(h), shh = spec_sin(h);
        const double nw = qw * chh - qz * shh, nz = qz * chh + qw * shh;
        const double n = sqrt(nw * nw + nz * nz);
        o.x = st->x + dt * o.vx;
        o.y = st->y + dt * o.vy;
        o.qw = nw / n; o.qz = nz / n;
        o.w[0] = L.wnew[c * 4]; o.w[1] = L.wnew[c * 4 + 1]; o.w[2] = L.wnew[c * 4 + 2]; o.w[3] = L.wnew[c * 4 + 3];
        L.next[c] = o;               // committed below, after every car of the workgroup has read its neighbours' pre-step states
    }
    wave_lds_sync();
    SUBSTAMP(3);
    {   // commit: the 13 doubles of the new dynamic state, spread over the car's four lanes
        if (on) {
            const double* src = reinterpret_cast<const double*>(L.next + c);
            double* dst = reinterpret_cast<double*>(st);
            for (int k = r; k < (int)(sizeof(Dyn) / sizeof(double)); k += 4) dst[k] = src[k];
            if (r == 0) L.steps[c] += 1;
        }
    }
    wave_lds_sync();
    SUBSTAMP(4);
    // ---- K3: distances = ((path - xpos)**2).sum(1); closest = distances.argmin() (first minimum), then the race-state update
    int idx; double best;
    bool upd = on && r == 0;             // the lane that updates the car's race state, its car slot and record
    int upd_c = c; CarCore* upd_st = st;
    if (ncars_here * 16 <= FTGP_WAVE) {
        // A small batch's workgroup holds at most four cars and its step IS the driver -> dynamics chain: sixteen lanes per car then walk seven
        // points each instead of four lanes twenty-five (lanes 14 and 15: two and none), and two more exchanges -- rotations by 8 and 4 inside the
        // row of 16 lanes -- bring every lane the car's first minimum.
        const int c16 = lane >> 4, q = lane & 15;
        const bool on16 = c16 < ncars_here;
        CarCore* st16 = L.cars + (on16 ? c16 : 0);
        const double x = st16->x, y = st16->y;
        const int first = q * 7, last = first + 7 < FTGP_PATH_POINTS ? first + 7 : FTGP_PATH_POINTS;
        idx = first < FTGP_PATH_POINTS ? first : 0x7fffffff; best = INFINITY;
        #pragma unroll 1
        for (int i = first; i < last; ++i) {
            const double dx = L.path[2 * i] - x, dy = L.path[2 * i + 1] - y;
            const double d = dx * dx + dy * dy;
            if (i == first || d < best) { best = d; idx = i; }
        }
        quad_argmin_step<0x128>(best, idx);      // row_ror:8
        quad_argmin_step<0x124>(best, idx);      // row_ror:4
        quad_argmin_step<0x4E>(best, idx);       // quad_perm [2,3,0,1]
        quad_argmin_step<0xB1>(best, idx);       // quad_perm [1,0,3,2]
        upd = on16 && q == 0; upd_c = c16; upd_st = st16;
    } else {
        const double x = st->x, y = st->y;
        idx = r * (FTGP_PATH_POINTS / 4);
        {
            const double dx = L.path[2 * idx] - x, dy = L.path[2 * idx + 1] - y;
            best = dx * dx + dy * dy;
        }
        #pragma unroll 1
        for (int i = idx + 1; i < (r + 1) * (FTGP_PATH_POINTS / 4); ++i) {
            const double dx = L.path[2 * i] - x, dy = L.path[2 * i + 1] - y;
            const double d = dx * dx + dy * dy;
            if (d < best) { best = d; idx = i; }
        }
        // the car's four lanes: exchanges inside the quad by DPP (quad_perm [1,0,3,2], then [2,3,0,1]), no LDS crossbar trip.
        // The lower index wins ties; a NaN never wins (the oracle's `d < best` is false for it too)
        quad_argmin_step<0xB1>(best, idx);
        quad_argmin_step<0x4E>(best, idx);
    }
    SUBSTAMP(5);
    if (upd) {
        Race rc; race_load(rc, upd_st);
        progress_update(P, rc, L.steps[upd_c], idx, best, P.cars[ci0 + upd_c].times, &upd_st->start);
        race_store(rc, upd_st);
    }
    wave_lds_sync();
    SUBSTAMP(6);
    // the LiDAR frames of the next step (its sweep starts after the workgroup barrier that ends this step)
    bool safe = true;
    if (on && r == 0) safe = frame_write(P, v, st, next_frames + c, c);
    const bool any_unsafe = __any(!safe);
    if (lane == 0) *unsafe_next = any_unsafe;
    SUBSTAMP(7);
    if (MULTI) {                     // env-mate records of the new frames: lane r of a car writes mates r and r + 4
        wave_lds_sync();
        const float cull = L.veh->cull_radius, r0f = (float)v.lidar_ring_radius;
        if (on) {
            pair_cull_write(next_frames, next_pairs, c, r, P.cars_per_env, cull, r0f);
            pair_cull_write(next_frames, next_pairs, c, r + 4, P.cars_per_env, cull, r0f);
        }
        wave_lds_sync();
        // (win_next: the next step's sweep draws from the window-only list -- its order lies right behind group_order)
        mate_masks(next_frames, next_pairs, next_mmask, P.mmask_stride, win_next ? order + FTGP_MAX_GROUPS : order, L.ray, P.n_rays, win_next ? P.win_tasks_per_car : P.tasks_per_car, P.cars_per_env, cull, P.group_cg, P.group_sg, ncars_here, lane, FTGP_WAVE);
    }
}

// Inclusive prefix sum over the 64 lanes of a wave with data-parallel-primitive moves (no LDS round trips): three shifts
// inside each row of 16 lanes, two more across its banks, then the row totals broadcast down (lane 15 of rows 0 and 2 into
// rows 1 and 3, lane 31 into rows 2 and 3).  A lane that a step does not address adds 0.
__device__ __forceinline__ int wave_inclusive_sum(int x)
{
    const int s1 = __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);      // row_shr:1
    const int s2 = __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);      // row_shr:2
    const int s3 = __builtin_amdgcn_update_dpp(0, x, 0x113, 0xf, 0xf, true);      // row_shr:3
    int v = x + s1 + s2 + s3;
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xe, true);                // row_shr:4, banks 1..3
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xc, true);                // row_shr:8, banks 2..3
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);                // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);                // row_bcast:31 into rows 2 and 3
    return v;
}

// Maximum / minimum over the 64 lanes of a wave, same moves, fused into the arithmetic: shifts by 1, 2, 4, 8 inside each row of
// 16 lanes leave a row's result in its lane 15, the two broadcasts carry it on; lane 63 holds the wave's.  A lane that a step
// does not address keeps its value.  (One asm statement each: the compiler emits move + DPP move + max per step; the waits
// are the two states a DPP read needs after the write of its source.)
#define FTGP_DPP_REDUCE(op) \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t" \
    "s_nop 1"
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
    asm volatile(FTGP_DPP_REDUCE("v_max_u32_dpp") : "+v"(x));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, FTGP_WAVE - 1);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
    asm volatile(FTGP_DPP_REDUCE("v_min_u32_dpp") : "+v"(x));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, FTGP_WAVE - 1);
}

// =============================================================================================
// K5: on-device drivers.  nidc.py:12-131 / fast.py:11-139 restated for one wave; the previous scan sits in LDS.
// =============================================================================================
// Number of points one disparity covers: ceil(2 * atan(width / (2 * close_dist)) / radians_per_point), nidc.py:57,93-99.
// close_dist is a binary32 sample and the count is a non-increasing step function of it, so the host tabulates -- with the
// very expression above, in binary64 with libm -- the largest sample thr[k] that still yields a count >= k (ftgp_create,
// build_cover_table).  The device then needs no atan: the count is the number of thresholds >= the sample.
// thr[0] holds the count for a sample of exactly 0 (the division by zero of the reference), as a float.
__device__ __forceinline__ int cover_count(const float* __restrict__ thr, int kmax, float close_dist, float half_width, float two_over_rpp)
{
    if (!(close_dist > 0.0f)) return close_dist == 0.0f ? (int)thr[0] : 0;      // negative (no hit) or NaN: nothing to cover
    // The answer is the largest k with thr[k] >= d (k = 0: none), and the table is the truth.  Seed k with the expression itself in
    // binary32 -- atan(x) ~ x / (1 + 0.28125 x^2), good to 0.005 rad for |x| <= 1 -- and walk to the answer: at most a step or two for
    // every sample a car can measure (a bisection of the table took eight rounds).  Any seed gives the same result.
    const float x = half_width * __builtin_amdgcn_rcpf(close_dist);
    const float a = x < 1.0f ? x * __builtin_amdgcn_rcpf(fmaf(0.28125f * x, x, 1.0f)) : 1.5707964f - __builtin_amdgcn_rcpf(x + 0.28125f * __builtin_amdgcn_rcpf(x));
    int k = (int)(a * two_over_rpp + 1.0f);
    k = k < 0 ? 0 : (k > kmax ? kmax : k);
    while (k < kmax && thr[k + 1] >= close_dist) ++k;
    while (k > 0 && thr[k] < close_dist) --k;
    return k;
}

// scan: [0] = ranges[0], [1 ...] = ranges[eighth : n - eighth] (the copy the reference makes, nidc.py:19, is this LDS row).
// Disparities are found on the unmodified scan (nidc.py:26-40) and extended in index order (nidc.py:86-105).  The cover
// counts (one atan each) are prepared for up to 64 disparities at once, one per lane; the ordered pass re-reads the two
// samples of each disparity and only recomputes the count when an earlier extension has changed them.
__device__ __forceinline__ void policy_disparity(const DriverShape& D, float* __restrict__ scan, CarCore* st, bool fast, int* __restrict__ list, const float* __restrict__ thr)
{
    const int lane = lane_here();
    const int n = D.n_rays;
    const double rpp = D.rpp;                                       // (2 pi) / n, nidc.py:121
    const int eighth = D.eighth;                                    // int(n / 8), nidc.py:18
    const int m = n - 2 * eighth;
    float* __restrict__ proc = scan + scan_window_first(eighth);
    const float range0 = scan[D.win_floats - 1];                    // ranges[0], fast.py:135
    const int kmax = D.cover_kmax;                                  // thr = the cover-count thresholds of this driver (width = (car_width / 2) * (1 + 300 / 100), nidc.py:93)
    const float half_width = fast ? 0.06f : 0.12f;                  // width / 2 = car_width (fast.py:4: 0.06, nidc.py:5: 0.12): seeds cover_count(), nothing else
    // Disparity flags (nidc.py:26-40, on the unmodified scan): lane l looks at samples l, 64 + l, 128 + l, ... (launch_steps()
    // guarantees m <= 64 * 64, i.e. K <= 64), so index order is (k, lane) order and a disparity's place in the ordered list is
    // the running total plus its rank among the flagged lanes of its k.  Disparities are rare: the common path of a k is two
    // LDS reads, a subtraction and ONE comparison (is anything at or above the threshold?); flags, ranks and list entries
    // are worked out only where that says yes.  Lanes past the end of the window (and sample 0, which has no predecessor)
    // read whatever lies there and are masked where it matters.
    // The reference compares |cur - prev| in binary64 with 0.6 (nidc.py:33).  In binary32, with T the float next above 0.6
    // (the nearest one): rounding is monotone, so |fl(cur - prev)| > T implies the exact difference is > 0.6 and < T implies it
    // is not; only a difference that rounds to exactly T needs the binary64 comparison (NaNs fail every test, as there).
    const int K = (m + FTGP_WAVE - 1) / FTGP_WAVE;
    SUBSTAMP_BEGIN();
    uint64_t mymask = 0;             // bit k: sample 64 k + lane is a disparity (needed again only beyond 64 disparities)
    int total = 0;                   // wave-uniform
    {
        const float T = 0.60000002384185791015625f;
        const float* __restrict__ p = proc + lane;                  // sample 64 k + lane is p[64 k]
        auto flagged = [&](int k, float cur, float prev, float ad) {    // some lane of group k is at or above the threshold
            const int i = k * FTGP_WAVE + lane;
            const bool valid = i >= 1 && i < m;
            bool fl = valid && ad > T;
            if (valid && ad == T) fl = fabs((double)cur - (double)prev) > 0.6;
            const uint64_t f = __builtin_amdgcn_ballot_w64(fl);
            if (fl) {
                const int r = total + rank_below(f);
                if (r < FTGP_WAVE) list[r] = i;
                mymask |= 1ull << k;
            }
            total += __popcll(f);
        };
        for (int k = 0; k < K; k += 2) {                            // two groups per trip: one address, two offsets
            const float cur0 = p[k * FTGP_WAVE], prev0 = p[k * FTGP_WAVE - 1];
            const float ad0 = fabsf(cur0 - prev0);
            if (__any(ad0 >= T)) flagged(k, cur0, prev0, ad0);
            if (k + 1 < K) {
                const float cur1 = p[(k + 1) * FTGP_WAVE], prev1 = p[(k + 1) * FTGP_WAVE - 1];
                const float ad1 = fabsf(cur1 - prev1);
                if (__any(ad1 >= T)) flagged(k + 1, cur1, prev1, ad1);
            }
        }
    }
    SUBSTAMP(8);
    for (int c0 = 0; c0 < total; c0 += FTGP_WAVE) {
        if (c0 > 0) {                // disparities c0 .. c0 + 63 of more than 64: their indices again, from the kept flags
            int run = 0;
            for (int k = 0; k < K; ++k) {
                const bool fl = ((mymask >> k) & 1ull) != 0;
                const uint64_t f = __builtin_amdgcn_ballot_w64(fl);
                if (fl) {
                    const int r = run + rank_below(f) - c0;
                    if (r >= 0 && r < FTGP_WAVE) list[r] = k * FTGP_WAVE + lane;
                }
                run += __popcll(f);
            }
        }
        wave_lds_sync();
        const int nchunk = total - c0 < FTGP_WAVE ? total - c0 : FTGP_WAVE;
        int index = 1; float q0 = 0.0f, q1 = 0.0f; int num = 0;
        if (lane < nchunk) {
            index = list[lane];
            q0 = proc[index - 1]; q1 = proc[index];
            num = cover_count(thr, kmax, (q1 < q0) ? q1 : q0, half_width, D.two_over_rpp);
        }
        wave_lds_sync();
        for (int d = 0; d < nchunk; ++d) {
            const int first = __builtin_amdgcn_readlane(index, d) - 1;
            const float p0v = proc[first], p1v = proc[first + 1];
            int nn = __builtin_amdgcn_readlane(num, d);
            const bool same = __float_as_uint(p0v) == (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(q0), d) &&
                              __float_as_uint(p1v) == (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(q1), d);
            const int close_idx = first + ((p1v < p0v) ? 1 : 0);   // argmin: first minimum
            const int far_idx = first + ((p1v > p0v) ? 1 : 0);     // argmax: first maximum
            const float ndf = (p1v < p0v) ? p1v : p0v;
            if (!__all(same)) nn = cover_count(thr, kmax, ndf, half_width, D.two_over_rpp);
            const bool cover_right = close_idx < far_idx;
            for (int i = lane; i < nn; i += FTGP_WAVE) {          // nidc.py:72-83, one target per lane
                const int idx = cover_right ? close_idx + 1 + i : close_idx - 1 - i;
                if (idx < 0 || idx >= m) break;
                if (proc[idx] > ndf) proc[idx] = ndf;
            }
            wave_lds_sync();
        }
    }
    wave_lds_sync();
    SUBSTAMP(9);
    // argmax, first maximum (nidc.py:127) = what the sequential loop "x > best" finds: every lane scans its own samples (l, 64 + l,
    // ...) in index order and remembers the GROUP of its best one (a wave-uniform number: no index arithmetic per sample); then
    // the wave's maximum, and the lowest index among the lanes that hold it.  Sample 0 is the running maximum to begin with,
    // whatever it is: a NaN there stays (like numpy's loop), NaNs elsewhere never win.
    float bv = -INFINITY; int bk = -1;
    if (lane == 0) { bv = proc[0]; bk = 0; }
    {
        const float* __restrict__ p = proc + lane;
        int k = 0;
        for (; k + 1 < K - 1; k += 2) {                             // groups before the last lie inside the window
            const float x0 = p[k * FTGP_WAVE], x1 = p[(k + 1) * FTGP_WAVE];
            if (x0 > bv) { bv = x0; bk = k; }
            if (x1 > bv) { bv = x1; bk = k + 1; }
        }
        if (k < K - 1) { const float x = p[k * FTGP_WAVE]; if (x > bv) { bv = x; bk = k; } }
        const float x = p[(K - 1) * FTGP_WAVE];
        if ((K - 1) * FTGP_WAVE + lane < m && x > bv) { bv = x; bk = K - 1; }
    }
    int bi;
    {
        // order-preserving integer image of the lane's maximum (-0 counts as +0, as it does for ">")
        const uint32_t b = __float_as_uint(bv + 0.0f);
        const uint32_t key = b ^ ((uint32_t)((int)b >> 31) | 0x80000000u);
        const uint32_t top = wave_max_u32(key);
        const uint32_t mine = (key == top && bk >= 0) ? (uint32_t)(bk * FTGP_WAVE + lane) : 0x7fffffffu;
        bi = (int)wave_min_u32(mine);
        const float b0 = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(bv)));
        if (b0 != b0) bi = 0;                                       // sample 0 is a NaN: nothing is greater
    }
    SUBSTAMP(10);
    double ang = ((double)bi - ((double)m / 2)) * rpp;              // nidc.py:112
    const double lim = 90.0 * (M_PI / 180.0);
    if (ang < -lim) ang = -lim;
    if (ang > lim) ang = lim;
    double speed, last = st->last_steer;
    if (!fast) {
        speed = 0.5 * 5 * (1 - fabs(ang) / (1.57 * 2));             // nidc.py:130
    } else {
        const double old = 0.0;                                     // fast.py:131-133
        ang = st->last_steer * old + ang * (1 - old);
        last = ang;
        if (fabs(ang) < 0.1 && (double)range0 > 0.5) speed = 7.0;   // fast.py:135-138
        else { const double sp = 0.5 * 5 * (1 - fabs(ang) / M_PI); speed = sp < 2.0 ? sp : 2.0; }
    }
    if (lane_id() == 0) { st->u_speed = speed; st->u_steer = ang; st->last_steer = last; }
    SUBSTAMP(11);
}

// evaluates the driver of car ci and stores the controls into its state record
__device__ __forceinline__ void policy_apply(const DeviceParams& P, const DriverShape& D, int policy, float* scan, CarCore* st, int ci, int64_t steps, int* list, const float* thr)
{
    const bool lane0 = lane_id() == 0;
    if (st->finished) {                                             // finished cars get the null driver (custom.py:1446)
        if (lane0) { st->u_speed = 0.0; st->u_steer = 0.0; }
        return;
    }
    switch (policy) {
    case FTGP_POLICY_LOBOTOMY: if (lane0) { st->u_speed = 0.0; st->u_steer = 0.0; } break;   // lobotomy.py:2-3
    case FTGP_POLICY_NIDC:
    case FTGP_POLICY_FAST: policy_disparity(D, scan, st, policy == FTGP_POLICY_FAST, list, thr); break;
    case FTGP_POLICY_RANDOM: {
        uint64_t h = splitmix64(P.seed + (uint64_t)((long)P.env_base * P.cars_per_env + ci) * 0x9E3779B97F4A7C15ull);
        h = splitmix64(h ^ (uint64_t)steps);
        if (lane0) { st->u_speed = 3.0 * u01(h); st->u_steer = 2.0 * u01(splitmix64(h)) - 1.0; }
        break; }
    default: break;
    }
}

// The network driver (include/ftgp.h "Network drivers"; the element operations: ftgp_net.h) of one car by one wave, lane = neuron:
//   inputs   input i lives in lane i % 64, register i / 64 (four registers: FTGP_NET_MAX_INPUTS = 256).  A lane forms the beams it owns
//            from the car's scan window in LDS -- pool reads and a running minimum each -- and the lanes that own a state input take
//            it from the car's record.
//   layer    lane j accumulates neurons j and j + 64 (FTGP_NET_MAX_HIDDEN = 128): acc = b[j], then for k ascending one fmaf with
//            x[k], which reaches all lanes as a scalar (v_readlane with a wave-uniform k), and Wt[k][j]: the wave's load of row k is one
//            coalesced segment per 64 neurons, shared by every car through L2.  The rows are independent of the accumulators, so the
//            unrolled loop has the loads of the rows ahead in flight under the fma chain, which is sequential by specification.
//   outputs  become the next layer's inputs in place: registers 0 and 1.
// No LDS beyond the window, no per-car state.  `win` is the address at which sample j of the car's scan sits when j is added.
#define FTGP_RIVAL_LANES 8             // lanes per env slot, in ftgp_io_rival_kernel and in the network driver's rival inputs
typedef const __attribute__((address_space(4))) NetDev* ScalarNet;
// rows [0, n) of one register's worth of inputs (n <= 64), FTGP_NET_AHEAD weights per lane at a time: the loads of the next rows are
// issued before the fma chain of the rows at hand (sixteen more in flight spill under the step kernel's 64 VGPRs)
#define FTGP_NET_AHEAD 6
template <bool WIDE>
__device__ __forceinline__ void net_rows(const float* __restrict__ row, int ld, int n, float xr, float& a0, float& a1)
{
    constexpr int U = WIDE ? FTGP_NET_AHEAD / 2 : FTGP_NET_AHEAD;
    float w0[U], w1[U];
    auto fetch = [&](float* d0, float* d1, int k) {
        #pragma unroll
        for (int u = 0; u < U; ++u) { d0[u] = row[(size_t)(k + u) * ld]; if (WIDE) d1[u] = row[(size_t)(k + u) * ld + FTGP_WAVE]; }
    };
    auto chain = [&](const float* s0, const float* s1, int k) {
        #pragma unroll
        for (int u = 0; u < U; ++u) {
            const float xk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xr), k + u));
            a0 = fmaf(s0[u], xk, a0);
            if (WIDE) a1 = fmaf(s1[u], xk, a1);
        }
    };
    int k = 0;
    if (n >= U) {
        fetch(w0, w1, 0);
        for (; k + 2 * U <= n; k += U) {
            float v0[U], v1[U];
            fetch(v0, v1, k + U);
            chain(w0, w1, k);
            #pragma unroll
            for (int u = 0; u < U; ++u) { w0[u] = v0[u]; if (WIDE) w1[u] = v1[u]; }
        }
        chain(w0, w1, k);
        k += U;
    }
    for (; k < n; ++k) {
        const float xk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xr), k));
        a0 = fmaf(row[(size_t)k * ld], xk, a0);
        if (WIDE) a1 = fmaf(row[(size_t)k * ld + FTGP_WAVE], xk, a1);
    }
}
// "Scan input" and "State input": the car's inputs into x, input i in lane i % 64 of register i / 64 (the act kernel records them)
// "Frame inputs" (ftgp_set_net_frame): the frame row of the car's record, entry j into the lane that owns input frame_first + j.  The wave
// has one car.  Search: lane l takes points l and l + 64 (l < 36) with K3's expression and keeps its first minimum; the pair (d, index)
// folds over xor-shuffles 1 .. 32 with the order "smaller d, then smaller index" (frame_nearer) -- the frame kernel's argument, widened
// from a row of sixteen to the wave: every lane ends with K3's first minimum.  (A NaN pose: every lane keeps its own (NaN, l), lane 0 has
// c = 0 as K3 does, and c is read from lane 0.)  Segment choice: lanes 0 and 1 project on segments B and A, and only g2 leaves them.
// Fixed entries: lanes 0 .. 3 project on the segment taken and lane k forms entry k -- one division in the code, not four side by side,
// whose temporaries do not fit the step kernel's 64 registers -- and v_readlane hands the four to the lanes that own those inputs.
// Look-ahead: the lane that owns an entry forms its pair and keeps its half.  The block is at most 36 wide, so a lane owns at most one
// entry.  The three phases hang on wave-uniform values (c, then the segment) in SGPRs, so what one phase computed is dead in the next.
// `path`: the centre-line of the car's track, LDS in the step kernel, device memory elsewhere.  Returns the lane's entry and, in reg,
// the register it belongs to (-1: the lane owns none).
__device__ __forceinline__ float net_frame_entry(const double* __restrict__ path, const CarCore* st, int first, int n_ahead, int stride, int& reg)
{
    const int lane = lane_here();
    int c;
    {
        const double px = st->x, py = st->y;
        double best = frame_dist2(path, lane, px, py); int idx = lane;
        if (lane < FTGP_PATH_POINTS - FTGP_WAVE) {
            const double d = frame_dist2(path, lane + FTGP_WAVE, px, py);
            if (d < best) { best = d; idx = lane + FTGP_WAVE; }
        }
        // (ds_bpermute at addresses formed here from lane_here(): __shfl_xor forms them from the lane counters, the optimiser moves the six
        // in front of the step loop and they end up in scratch memory under the step kernel's 64 registers)
        #pragma unroll
        for (int m = 1; m < FTGP_WAVE; m <<= 1) {
            const int from = (lane ^ m) << 2;
            const double od = __hiloint2double(__builtin_amdgcn_ds_bpermute(from, __double2hiint(best)), __builtin_amdgcn_ds_bpermute(from, __double2loint(best)));
            const int oi = __builtin_amdgcn_ds_bpermute(from, idx);
            if (frame_nearer(od, oi, best, idx)) { best = od; idx = oi; }
        }
        c = __builtin_amdgcn_readfirstlane(idx);
    }
    const int pa = c > 0 ? c - 1 : FTGP_PATH_POINTS - 1;
    int seg;
    {
        double g2 = 0.0;
        if (lane < 2) g2 = frame_segment(path, lane == 0 ? c : pa, st->x, st->y).g2;
        const double g2b = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(g2), 0), __builtin_amdgcn_readlane(__double2loint(g2), 0));
        const double g2a = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(g2), 1), __builtin_amdgcn_readlane(__double2loint(g2), 1));
        seg = __builtin_amdgcn_readfirstlane(g2a < g2b ? pa : c);        // A only if strictly nearer
    }
    const double qw = st->qw, qz = st->qz;
    const double ch = qw * qw - qz * qz, sh = 2.0 * (qw * qz);
    float e = 0.0f;
    if (lane < FTGP_FRAME_FIXED) {
        double s;
        e = frame_fixed_entry(frame_segment(path, seg, st->x, st->y), seg, ch, sh, lane, s);
    }
    const int j = (lane - first) & (FTGP_WAVE - 1);               // the entry this lane owns, if j < width
    reg = j < FTGP_FRAME_FIXED + 2 * n_ahead ? (first + j) >> 6 : -1;
    const int ei = __float_as_int(e);
    float v = __int_as_float(j == 0 ? __builtin_amdgcn_readlane(ei, 0) : j == 1 ? __builtin_amdgcn_readlane(ei, 1) : j == 2 ? __builtin_amdgcn_readlane(ei, 2)
                                                                                                                            : __builtin_amdgcn_readlane(ei, 3));
    if (j >= FTGP_FRAME_FIXED && reg >= 0) {
        const FramePoint p = frame_ahead(path, seg, (j - FTGP_FRAME_FIXED) >> 1, stride, st->x, st->y, ch, sh);
        v = (j & 1) ? p.y : p.x;
    }
    return v;
}
// "Rival inputs" (ftgp_set_net_rivals): the rival row of the car in slot `slot` of its env, entry j into the lane that owns input
// rival_first + j.  The wave has one car a and reads every car of the env where its record lies (`cars`: the env's slot 0 -- the
// workgroup's LDS in the step kernel, device memory elsewhere).  Eight lanes per env slot, as ftgp_io_rival_kernel groups them: lane
// (b, i) = 8 b + i.
//   search    lane (b, i) walks points i, i + 8, ... of the path for car b with K3's expression and keeps its first minimum; the pair
//             folds over xor 1, 2, 4 with frame_nearer: lane (b, 0) ends with K3's first minimum (a NaN pose: every lane keeps its own,
//             lane (b, 0) has c = 0 as K3 does), and c is taken from that lane.
//   segment   lanes (b, 0) and (b, 1) project on segments B and A; only t and g2 leave lane (b, 1).  Lane (b, 0) forms s_b, off_b, g_b
//             and hands s_b and g_b to its group.
//   a         car a's s and g reach all lanes by v_readlane at the wave-uniform lane 8 slot.
//   place     place, n_racing and the mates are ballots and popcounts over the lanes (b, 0); the two gaps are minima folded over xor 8,
//             16, 32 (the eight lanes of a group hold the same value).
//   rank      lane (b, i) asks whether mate i comes before mate b in (d2, slot) order; a ballot gives mate b its rank as the popcount of
//             byte b.
//   entries   lane (b, q) forms entry q of mate b (rival_mate_entry) and, if b's rank is below n_rivals, sends it to the lane that owns
//             that input -- a forward permute; every other lane sends to the lane 63 places behind rival_first, which owns no rival
//             entry since the block is at most 60 wide.  A lane nobody sends to receives 0: the slot without a mate.
// The phases hang on values in SGPRs (the slot, the ballots) and on s_b, g_b; the addresses of the permutes are formed on the spot (see
// net_frame_entry).  Nothing here reads the controls, so in the step kernel no barrier is needed: dynamics_lanes() runs only after every
// driver of the workgroup has delivered, and until then every record's pose, velocity, completion and finish fields are the previous
// step's.  Returns the lane's entry and, in reg, the register it belongs to (-1: the lane owns none).
__device__ __forceinline__ int32_t absolute_completion(const CarCore& a);
__device__ __forceinline__ RivalCar rival_car(const CarCore& r, double s) { return rival_car(r.x, r.y, r.qw, r.qz, r.vx, r.vy, s); }
__device__ __forceinline__ double net_pull_f64(int from, double v)
{
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(from, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(from, __double2loint(v)));
}
// the centre-line of the car's track; the record of its env's slot 0 and the bytes from one record to the next (CarCore in LDS, CarState in
// device memory); its slot; cars per env
struct NetEnv { const double* path; const CarCore* cars; int stride, slot, cpe; };
__device__ __forceinline__ const CarCore* net_env_car(const NetEnv& E, int k) { return reinterpret_cast<const CarCore*>(reinterpret_cast<const unsigned char*>(E.cars) + (size_t)k * E.stride); }
__device__ __forceinline__ float net_rival_entry(const NetEnv E, int first, int n_rivals, int& reg)
{
    const int lane = lane_here();
    const int b = lane >> 3, i = lane & (FTGP_RIVAL_LANES - 1);
    const int slot = __builtin_amdgcn_readfirstlane(E.slot), cpe = __builtin_amdgcn_readfirstlane(E.cpe);
    const bool has = b < cpe;
    const CarCore* rb = net_env_car(E, has ? b : slot);      // (a group that holds nobody reads a's record: in bounds, and nothing of it is used)
    const double* __restrict__ path = E.path;
    double s_b, g_b;
    {
        const double px = rb->x, py = rb->y;
        double best = frame_dist2(path, i, px, py); int idx = i;
        #pragma unroll 1
        for (int p = i + FTGP_RIVAL_LANES; p < FTGP_PATH_POINTS; p += FTGP_RIVAL_LANES) {
            const double d = frame_dist2(path, p, px, py);
            if (d < best) { best = d; idx = p; }
        }
        #pragma unroll
        for (int m = 1; m < FTGP_RIVAL_LANES; m <<= 1) {
            const int from = (lane ^ m) << 2;
            const double od = net_pull_f64(from, best);
            const int oi = __builtin_amdgcn_ds_bpermute(from, idx);
            if (frame_nearer(od, oi, best, idx)) { best = od; idx = oi; }
        }
        const int head = (lane & ~(FTGP_RIVAL_LANES - 1)) << 2;
        const int c = __builtin_amdgcn_ds_bpermute(head, idx);
        const int pa = c > 0 ? c - 1 : FTGP_PATH_POINTS - 1;
        double t = 0.0, g2 = 0.0;
        if (i < 2) { const FrameSeg g = frame_segment(path, i == 0 ? c : pa, px, py); t = g.t; g2 = g.g2; }
        const double ta = net_pull_f64(head + 4, t), g2a = net_pull_f64(head + 4, g2);
        const bool take_a = g2a < g2;                    // A only if strictly nearer
        double s = (double)(take_a ? pa : c) + (take_a ? ta : t);
        if (s >= 100.0) s = s - 100.0;
        const double g = rival_progress(absolute_completion(*rb), s, c, best > 1.0);
        s_b = net_pull_f64(head, s); g_b = net_pull_f64(head, g);
    }
    const int la = slot * FTGP_RIVAL_LANES;
    const double s_a = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s_b), la), __builtin_amdgcn_readlane(__double2loint(s_b), la));
    const double g_a = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(g_b), la), __builtin_amdgcn_readlane(__double2loint(g_b), la));
    const CarCore* ra = net_env_car(E, slot);
    const bool fin_a = ra->finished != 0, fin_b = rb->finished != 0;
    const bool other = has && b != slot;
    const bool ahead = other && rival_ahead(fin_b, rb->finish_step, g_b, b, fin_a, ra->finish_step, g_a, slot);
    const bool mate = other && !fin_b && !fin_a;
    const int place = 1 + __builtin_popcountll(__builtin_amdgcn_ballot_w64(ahead && i == 0));
    const int n_racing = __builtin_popcountll(__builtin_amdgcn_ballot_w64(has && !fin_b && i == 0));
    float fixed;
    {
        double gap_ahead = (mate && ahead) ? g_b - g_a : INFINITY;
        double gap_behind = (mate && !ahead) ? g_a - g_b : INFINITY;
        #pragma unroll
        for (int m = FTGP_RIVAL_LANES; m < FTGP_WAVE; m <<= 1) {
            const int from = (lane ^ m) << 2;
            const double oa = net_pull_f64(from, gap_ahead), ob = net_pull_f64(from, gap_behind);
            if (oa < gap_ahead) gap_ahead = oa;
            if (ob < gap_behind) gap_behind = ob;
        }
        const float f2 = gap_ahead == INFINITY ? 0.0f : (float)gap_ahead, f3 = gap_behind == INFINITY ? 0.0f : (float)gap_behind;
        const int j = (lane - first) & (FTGP_WAVE - 1);
        fixed = j == 0 ? (float)place : j == 1 ? (float)n_racing : j == 2 ? f2 : f3;
    }
    const RivalCar a = rival_car(*ra, s_a), m = rival_car(*rb, s_b);
    int rank;
    {
        const double dx = m.x - a.x, dy = m.y - a.y;
        const double d2 = dx * dx + dy * dy;
        const uint64_t mates = __builtin_amdgcn_ballot_w64(mate);
        const double od = net_pull_f64(i << 5, d2);      // lane (i, 0)
        const bool before = ((mates >> (i * FTGP_RIVAL_LANES)) & 1) != 0 && (od < d2 || (od == d2 && i < b));
        const uint64_t bal = __builtin_amdgcn_ballot_w64(before);
        rank = __builtin_popcount((uint32_t)(bal >> (b * FTGP_RIVAL_LANES)) & 0xffu);
    }
    const float e = rival_mate_entry(a, m, i);
    const int to = (mate && rank < n_rivals) ? first + FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * rank + i : first + FTGP_WAVE - 1;
    float v = __int_as_float(__builtin_amdgcn_ds_permute((to & (FTGP_WAVE - 1)) << 2, __float_as_int(e)));
    const int j = (lane - first) & (FTGP_WAVE - 1);               // the entry this lane owns, if j < width
    reg = j < FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * n_rivals ? (first + j) >> 6 : -1;
    if (j < FTGP_RIVAL_FIXED) v = fixed;
    return v;
}
// env(): the centre-line of the car's track, the records of its env and its slot there, asked for by a slot with frame or rival inputs
// only (elsewhere than in the step kernel the path costs a scalar load and a wait, which a launch without such inputs does not pay)
template <class EnvFn>
__device__ __forceinline__ void net_inputs(const ScalarNet N, const float* __restrict__ win, const CarCore* st, EnvFn env, float (&x)[4])
{
    const int lane = lane_here();
    // (the rival entry before everything else: its binary64 then has the registers to itself)
    const int rshape = N->rival_shape;
    int rival_reg = -1;
    float rival_v = 0.0f;
    if (rshape != 0) rival_v = net_rival_entry(env(), N->rival_first, rshape >> 8, rival_reg);      // wave-uniform: the slot's record
    const int pool = N->pool, n_beams = N->n_beams;
    const float M = N->max_range, inv = N->inv_max_range;
    // (the frame entry first: its binary64 then has the registers to itself, not the four of x as well)
    const int shape = N->frame_shape;
    int frame_reg = -1;
    float frame_v = 0.0f;
    if (shape != 0) frame_v = net_frame_entry(env().path, st, N->frame_first, shape & 0xff, shape >> 8, frame_reg);   // wave-uniform: the slot's record
    x[0] = 0.0f; x[1] = 0.0f; x[2] = 0.0f; x[3] = 0.0f;
    {
        const float* __restrict__ mine = win + (N->beam_first + lane) * pool;
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r * FTGP_WAVE < n_beams && r * FTGP_WAVE + lane < n_beams) x[r] = ftgp_net_beam(mine + r * FTGP_WAVE * pool, pool, M, inv);
    }
    if (N->use_state) {
        #pragma unroll
        for (int q = 0; q < FTGP_NET_STATE_INPUTS; ++q) {
            const float v = ftgp_net_state(q, st->qw, st->qz, st->vx, st->vy, st->wz, st->u_speed, st->u_steer);
            const int i = n_beams + q;
            #pragma unroll
            for (int r = 0; r < 4; ++r) if ((i >> 6) == r && lane == (i & (FTGP_WAVE - 1))) x[r] = v;
        }
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) if (frame_reg == r) x[r] = frame_v;
    #pragma unroll
    for (int r = 0; r < 4; ++r) if (rival_reg == r) x[r] = rival_v;
}
// "Layers": x becomes the outputs of the last layer, y0 in lane 0 and y1 in lane 1 of x[0]
// A slot with a population (ftgp_set_net_population): the parameters are those of the member of the car's env, one more wave-uniform
// scalar -- params + env_member[env] * stride, two scalar loads ahead of the first row.  env_of(): the car's env in the handle, asked
// for by such a slot only.
template <class EnvOf>
__device__ __forceinline__ void net_layers(const ScalarNet N, EnvOf env_of, float (&x)[4])
{
    const int lane = lane_here();
    const float* __restrict__ params = uniform_ptr(N->params);
    if (const int32_t* map = N->env_member) {
        const int member = __builtin_amdgcn_readfirstlane(uniform_ptr(map)[__builtin_amdgcn_readfirstlane(env_of())]);
        params = uniform_ptr(params + (size_t)member * (size_t)net_member_stride(N->n_floats));
    }
    const int n_layers = N->n_layers;
    for (int l = 0; l < n_layers; ++l) {
        const int n_in = N->width[l], n_out = N->width[l + 1];
        const int ld = (n_out + FTGP_WAVE - 1) & ~(FTGP_WAVE - 1);
        const float* __restrict__ W = params + N->w_off[l] + lane;
        const float* __restrict__ B = params + N->b_off[l] + lane;
        float a0 = B[0], a1 = 0.0f;
        if (ld > FTGP_WAVE) {
            a1 = B[FTGP_WAVE];
            #pragma unroll
            for (int r = 0; r < 4; ++r) if (r * FTGP_WAVE < n_in) net_rows<true>(W + (size_t)r * FTGP_WAVE * ld, ld, min(FTGP_WAVE, n_in - r * FTGP_WAVE), x[r], a0, a1);
        } else {
            #pragma unroll
            for (int r = 0; r < 4; ++r) if (r * FTGP_WAVE < n_in) net_rows<false>(W + (size_t)r * FTGP_WAVE * ld, ld, min(FTGP_WAVE, n_in - r * FTGP_WAVE), x[r], a0, a1);
        }
        const int act = l + 1 < n_layers ? N->hidden_act : N->out_act;
        x[0] = ftgp_net_act(act, a0); x[1] = 0.0f; x[2] = 0.0f; x[3] = 0.0f;
        if (ld > FTGP_WAVE) x[1] = ftgp_net_act(act, a1);
    }
}
// the record of slot `slot` behind scalar loads
__device__ __forceinline__ ScalarNet scalar_net(const NetDev* table, int slot)
{
    uint64_t ta = (uint64_t)(table + slot); asm volatile("" : "+s"(ta));
    return (ScalarNet)ta;
}
template <class EnvFn, class EnvOf>
__device__ __forceinline__ void policy_net(const NetDev* table, int slot, const float* __restrict__ win, CarCore* st, EnvFn env, EnvOf env_of)
{
    const ScalarNet N = scalar_net(table, slot);
    const int lane = lane_here();
    float x[4];
    net_inputs(N, win, st, env, x);
    net_layers(N, env_of, x);
    const float y0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[0]), 0)), y1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[0]), 1));
    const float scale[2] = { N->out_scale[0], N->out_scale[1] }, offset[2] = { N->out_offset[0], N->out_offset[1] };
    double us, ut;
    ftgp_net_controls(y0, y1, scale, offset, &us, &ut);
    if (lane == 0) { st->u_speed = us; st->u_steer = ut; }
}
// the driver FTGP_POLICY_NET0 + slot of one car: a finished car gets the null driver before the network is looked at
template <class EnvFn, class EnvOf>
__device__ __forceinline__ void policy_apply_net(const NetDev* table, int slot, const float* scan, int eighth, CarCore* st, EnvFn env, EnvOf env_of)
{
    if (st->finished) {
        if (lane_id() == 0) { st->u_speed = 0.0; st->u_steer = 0.0; }
        return;
    }
    policy_net(table, slot, scan + scan_window_first(eighth) - eighth, st, env, env_of);
}

// =============================================================================================
// End-of-launch metrics record (FTGP_METRIC_DOUBLES; the record ftgp_metrics_kernel computes from the state in HBM), folded into
// the step kernel so that a launch needs no second kernel and no second synchronisation: every workgroup reduces its own cars
// and publishes the partial record; the workgroup that arrives last adds the partials up.  The sums are integers, exact in
// binary64 in any order, so the result is bit-identical to the separate kernel's.  Hand-off between workgroups in the counter
// form of the CDNA guide with write-through stores: ONE lane stores its workgroup's record with agent-scope (sc1) stores, waits
// for them and draws a ticket (relaxed agent-scope fetch_add); the workgroup that draws the last ticket takes an agent-scope
// acquire fence, waits, passes a barrier and reads the records.  (A release fence per workgroup instead -- an L2 write-back
// each -- cost 14 us per launch, as much as the separate kernel.  Tickets in two levels -- eight per-XCD counters, then a top one --
// changed nothing: what this costs per launch -- 5 us since the reductions are DPP moves and the last workgroup reads the records with one
// thread each -- is three dependent trips to memory (the record's stores, the ticket, the last workgroup's read), not the 512 atomics on one word.)
__device__ __forceinline__ double wave_sum_f64(double v)
{
    #pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
    return v;
}

// The same reductions with data-parallel-primitive moves (no LDS round trips; the wave's result comes out of lane 63): the end-of-launch
// record is on every launch's critical tail, and six sums + a min + a max by __shfl_xor are 96 LDS crossbar trips.
// one step: every lane receives the value of the lane CTRL names; a lane the step does not address (or whose source lies outside the
// row) sees the identity: +0 for the sums (old = 0, bound_ctrl), its own value for min / max (old = itself)
template <int CTRL, int ROW_MASK, int BANK_MASK, bool KEEP_OWN>
__device__ __forceinline__ double dpp_moved_f64(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int mlo, mhi;
    if (KEEP_OWN) { mlo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, BANK_MASK, false); mhi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, BANK_MASK, false); }
    else          { mlo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, BANK_MASK, true);   mhi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, BANK_MASK, true); }
    return __hiloint2double(mhi, mlo);
}
template <bool KEEP_OWN, class Op>
__device__ __forceinline__ double wave_reduce_f64_dpp(double x, Op op)
{
    double v = x;
    v = op(v, dpp_moved_f64<0x111, 0xf, 0xf, KEEP_OWN>(v));      // row_shr:1   -- after the four shifts lane 15 of every row holds the row's result
    v = op(v, dpp_moved_f64<0x112, 0xf, 0xf, KEEP_OWN>(v));      // row_shr:2
    v = op(v, dpp_moved_f64<0x114, 0xf, 0xf, KEEP_OWN>(v));      // row_shr:4
    v = op(v, dpp_moved_f64<0x118, 0xf, 0xf, KEEP_OWN>(v));      // row_shr:8
    v = op(v, dpp_moved_f64<0x142, 0xa, 0xf, KEEP_OWN>(v));      // row_bcast:15 into rows 1 and 3
    v = op(v, dpp_moved_f64<0x143, 0xc, 0xf, KEEP_OWN>(v));      // row_bcast:31 into rows 2 and 3
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), FTGP_WAVE - 1), __builtin_amdgcn_readlane(__double2loint(v), FTGP_WAVE - 1));
}
__device__ __forceinline__ double wave_total_f64(double x) { return wave_reduce_f64_dpp<false>(x, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ double wave_least_f64(double x) { return wave_reduce_f64_dpp<true>(x, [](double a, double b) { return fmin(a, b); }); }
__device__ __forceinline__ double wave_most_f64(double x) { return wave_reduce_f64_dpp<true>(x, [](double a, double b) { return fmax(a, b); }); }

// One rank and no communicator (HOST_SUM: bit 1 of the launch's slot argument): nothing on the device needs the launch's record, so every
// workgroup writes its partial record straight to pinned host memory -- [slot][workgroup][FTGP_METRIC_DOUBLES] -- and is done: no ticket, no
// last workgroup, no barrier; the host adds the partial records up when the record is asked for (collect_slot() in ftgp_api.hip: integers,
// exact in any order, bit-identical again).  That takes the hand-off's three dependent trips to memory out of every launch's tail.
// called by ALL threads of the workgroup, after the state records have gone back to HBM; `scratch`: one int of LDS
template <bool HOST_SUM>
__device__ __forceinline__ void launch_metrics(const DeviceParams& P, const CarCore* cars_lds, const int64_t* steps_lds, int ncars_here, int ci0,
                                               unsigned char* scratch, double* partial /* [waves][FTGP_METRIC_DOUBLES] of LDS */, int slot, int wave)
{
    int* last_flag = reinterpret_cast<int*>(scratch);
    const int lane = lane_id();
    if (HOST_SUM && wave != 0) return;
    if (wave == 0) {                       // wave 0: one car per lane (a workgroup holds at most 16)
        double v[7] = { 0, 0, 0, 0, 0, INFINITY, -INFINITY };      // steps, laps, absolute completion, finished, off track, min / max lap time
        if (lane < ncars_here) {
            const CarCore* a = cars_lds + lane;
            const int ci = ci0 + lane;
            const int lc = a->good_start ? a->completion : -(100 - a->completion);     // custom.py:132-143
            if (ci % P.cars_per_env == 0) v[0] = (double)steps_lds[lane];
            v[1] = a->laps; v[2] = a->laps * 100 + lc; v[3] = a->finished; v[4] = a->off_track;
            const int n = a->n_times < FTGP_MAX_LAP_TIMES ? a->n_times : FTGP_MAX_LAP_TIMES;      // the ring's occupied slots
            const double* t = P.cars[ci].times;
            for (int k = 0; k < n; ++k) { v[5] = fmin(v[5], t[k]); v[6] = fmax(v[6], t[k]); }
        }
        #pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = wave_total_f64(v[q]);
        v[5] = wave_least_f64(v[5]); v[6] = wave_most_f64(v[6]);
        if (HOST_SUM) {
            if (lane == 0) {
                double* mine = P.wg_metrics_host + ((size_t)slot * gridDim.x + blockIdx.x) * FTGP_METRIC_DOUBLES;
                const double rec[FTGP_METRIC_DOUBLES] = { v[0], (double)ncars_here, v[1], v[2], v[3], v[4], v[5], v[6] };
                #pragma unroll
                for (int q = 0; q < FTGP_METRIC_DOUBLES; ++q) mine[q] = rec[q];
            }
            return;
        }
        if (lane == 0) {
            // the one lane that publishes also counts: write-through (agent-scope) stores of the record, wait for them, then the ticket
            double* mine = P.wg_metrics + (size_t)blockIdx.x * FTGP_METRIC_DOUBLES;
            const double rec[FTGP_METRIC_DOUBLES] = { v[0], (double)ncars_here, v[1], v[2], v[3], v[4], v[5], v[6] };
            #pragma unroll
            for (int q = 0; q < FTGP_METRIC_DOUBLES; ++q) __hip_atomic_store(mine + q, rec[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned int ticket = __hip_atomic_fetch_add(P.wg_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *last_flag = ticket == gridDim.x - 1;
        }
    }
    __syncthreads();
    if (!*last_flag) return;                              // workgroup-uniform
    if (wave == 0 && lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // every thread of the last workgroup takes records (one thread per workgroup of the grid: the loads of a record are in flight together and
    // the whole read costs one memory latency), each wave reduces its lanes by DPP, wave 0 reduces the waves' results
    static_assert(sizeof(double) * 2 * FTGP_PATH_POINTS >= 16 * FTGP_METRIC_DOUBLES * sizeof(double), "the centre line's LDS bytes hold the waves' partial records");
    const int nwaves = (int)(blockDim.x >> 6);
    {
        double v[FTGP_METRIC_DOUBLES] = { 0, 0, 0, 0, 0, 0, INFINITY, -INFINITY };
        for (unsigned int b = (unsigned int)(wave * FTGP_WAVE + lane); b < gridDim.x; b += blockDim.x) {      // (threadIdx.x itself would be one more register held from the kernel's first instruction to here)
            const double* r = P.wg_metrics + (size_t)b * FTGP_METRIC_DOUBLES;
            #pragma unroll
            for (int q = 0; q < 6; ++q) v[q] += r[q];
            v[6] = fmin(v[6], r[6]); v[7] = fmax(v[7], r[7]);
        }
        if ((unsigned int)wave * FTGP_WAVE < gridDim.x) {                 // waves without a record have nothing to add (workgroup-uniform per wave)
            #pragma unroll
            for (int q = 0; q < 6; ++q) v[q] = wave_total_f64(v[q]);
            v[6] = wave_least_f64(v[6]); v[7] = wave_most_f64(v[7]);
        }
        if (lane == 0) {
            #pragma unroll
            for (int q = 0; q < FTGP_METRIC_DOUBLES; ++q) partial[wave * FTGP_METRIC_DOUBLES + q] = v[q];
        }
    }
    __syncthreads();
    if (wave == 0) {
        double v[FTGP_METRIC_DOUBLES] = { 0, 0, 0, 0, 0, 0, INFINITY, -INFINITY };
        if (lane < nwaves) {
            #pragma unroll
            for (int q = 0; q < FTGP_METRIC_DOUBLES; ++q) v[q] = partial[lane * FTGP_METRIC_DOUBLES + q];
        }
        #pragma unroll
        for (int q = 0; q < 6; ++q) v[q] = wave_total_f64(v[q]);
        v[6] = wave_least_f64(v[6]); v[7] = wave_most_f64(v[7]);
        if (lane == 0) {
            #pragma unroll
            for (int q = 0; q < FTGP_METRIC_DOUBLES; ++q) { P.metrics_dev[slot * FTGP_METRIC_DOUBLES + q] = v[q]; P.metrics_host[slot * FTGP_METRIC_DOUBLES + q] = v[q]; }
            __hip_atomic_store(P.wg_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next launch counts from zero again
        }
    }
}

// =============================================================================================
// The step kernel.  Per step and car, in the order of the reference loop (custom.py:1337-1426):
//   driver(previous scan) -> ctrl -> [mj_step: sensors at the current pose, integrate] -> steps += 1 ->
//   progress at the new pose (= the head of the next loop iteration).
// =============================================================================================
__device__ __forceinline__ void stage16(void* dst, const void* src, int bytes)
{
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const int n = bytes >> 4;
    for (int i = threadIdx.x; i < n; i += blockDim.x) d4[i] = s4[i];
}

#ifndef FTGP_WAVES_PER_EU
#define FTGP_WAVES_PER_EU 8       // two 16-wave workgroups per CU: at most 64 VGPRs per lane
#endif
// MULTI: several cars per env (inter-vehicle rays and contacts).  FAKE: FTGP_LIDAR_FAKELIDAR -- the sweep is lidar_fake() (its own
// instantiation, so that the rangefinder kernels' code generation does not move).  metrics_slot: which of the two record slots this
// launch's metrics go to (ftgp_metrics_allgather_begin / _end); bit 1: the workgroups' partial records go to pinned host memory (launch_metrics).
// ROSTER: `policy` may be FTGP_POLICY_PER_CAR (every car slot its own driver, ftgp_set_car_policies) -- again its own instantiation, so
// that the single-driver kernels stay exactly what they were (the multi-car one lost 3 % to the run-time form of this test); the
// FAKELIDAR kernels, which are for parity and not for throughput, exist in the ROSTER form only.
// TRACKS: the instantiations of multi-track handles (ftgp_create_tracks): the workgroups of a launch race different tracks, each workgroup
// one.  With TRACKS = false the code is exactly the one-track kernel's.
// DYN: launches with the table of per-car dynamics on (ftgp_set_dynamics) -- their own instantiations once more, MULTI x ROSTER x TRACKS with
// FAKE = false: the workgroup stages its cars' records into LDS behind the layout, at lds_bytes (the launch asks for cars_per_block records
// more), and dynamics_lanes() reads them.  With DYN = false the code is exactly what it was.
// NET: launches whose policy, roster or device-io slot table names a network driver (FTGP_POLICY_NET0 ..., ftgp_set_net) -- ROSTER form
// only, FAKE = false, MULTI x TRACKS x DYN: `policy` may then be a network's number (every car) or FTGP_POLICY_PER_CAR with networks
// among the slots; policy_net() is one more case of K5.  With NET = false the code is exactly what it was.
template <bool MULTI, bool FAKE, bool ROSTER, bool TRACKS, bool DYN = false, bool NET = false>
__global__ void __launch_bounds__(1024, FTGP_WAVES_PER_EU) ftgp_step_kernel(const DeviceParams* __restrict__ Pg, int policy, int n_steps, int metrics_slot)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // TRACKS: Pg is track 0's parameter block.  The workgroup's entry in the table behind it (ftgp_create_tracks) names the block of the
    // workgroup's track, Pt (byte offset from track 0's), its first car and its number of cars: scalar loads, once per launch.  From here
    // on the workgroup runs the one-track code on its track's staging image and block.  (The LDS layout is the same in every block: the
    // offsets are read from Pg, as with one track.)
    const DeviceParams* Pt = Pg;
    int wg_first = 0, wg_cars = 0;
    if (TRACKS) {
        typedef const __attribute__((address_space(4))) int* ScalarInts4;
        const ScalarInts4 ent = reinterpret_cast<ScalarInts4>(reinterpret_cast<uint64_t>(Pg) + FTGP_PARAMS_BYTES) + 4 * blockIdx.x;
        Pt = reinterpret_cast<const DeviceParams*>(reinterpret_cast<const unsigned char*>(Pg) + ent[0]);
        wg_first = ent[1]; wg_cars = ent[2];
    }
    const DeviceParams& P0 = *reinterpret_cast<const DeviceParams*>(lds + Pg->off_params);   // valid after staging + barrier
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = __builtin_amdgcn_readfirstlane(blockDim.x >> 6);
    FTGP_DIAG_WG_ENTER();
    // The parameter block itself goes to LDS (later reads come from there, not from ~70 pinned SGPRs), with the vehicle constants, the centre
    // line, the fan and the driver's cover table: ONE image in HBM laid out as the LDS is (ftgp_create), so that a thread's loads are all in
    // flight together -- the launch pays one memory latency here, not one per table.
    {
        // (the cover table of the launch's driver; FTGP_POLICY_PER_CAR: both, nidc's first)
        const int head = Pg->off_cars - Pg->off_params;
        const int cover = (policy == FTGP_POLICY_NIDC || policy == FTGP_POLICY_FAST) ? Pg->stage_cover : (ROSTER && policy == FTGP_POLICY_PER_CAR) ? 2 * Pg->stage_cover : 0;
        const uint4* img = reinterpret_cast<const uint4*>(TRACKS ? scalar_view(Pt)->stage_img : Pg->stage_img);
        const uint4* cov = img + ((head + (policy == FTGP_POLICY_FAST ? Pg->stage_cover : 0)) >> 4);
        uint4* d_head = reinterpret_cast<uint4*>(lds + Pg->off_params);
        uint4* d_cov = reinterpret_cast<uint4*>(lds + Pg->off_cover);
        const int nh = head >> 4, n = nh + (cover >> 4);
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            if (i < nh) d_head[i] = img[i];
            else d_cov[i - nh] = cov[i - nh];
        }
    }
    if (threadIdx.x < 8) reinterpret_cast<int*>(lds + Pg->off_pool)[threadIdx.x] = 0;
    __syncthreads();
    const LdsOffsets off = lds_offsets(P0);
    const int cpb = sgpr(P0.cars_per_block);
    const int ci0 = TRACKS ? wg_first : FTGP_DIAG_WG_GROUP((int)blockIdx.x) * cpb;
    const int ncars_here = TRACKS ? wg_cars : min(cpb, sgpr(P0.n_cars) - ci0);
    const bool second_half = (((int)blockIdx.x / max(1, sgpr(P0.n_cu))) & 1) != 0;      // see sweep_priority(): workgroups b and b + n_cu share a CU in the first dispatch wave
    // (a NET launch's policy is a network's number or FTGP_POLICY_PER_CAR: its drivers read the scan)
    const bool need_scan = NET ? true : (policy == FTGP_POLICY_NIDC || policy == FTGP_POLICY_FAST || (ROSTER && policy == FTGP_POLICY_PER_CAR));
    {
    const DeviceParams& P = P0;
    const Lds L = lds_view(off, lds);
    const int R = P.n_rays, eighth = P.eighth, win_floats = P.win_floats;
    if (need_scan) {     // the scan of the previous launch is what the first driver call sees: buffer 1 = parity of step -1.  All waves fetch it,
                         // a thread's loads (one per car) in flight together; the first driver call is on the launch's critical path
        const int nwin = R - 2 * eighth;
        for (int j = (int)threadIdx.x; j < nwin; j += (int)blockDim.x) {
            #pragma unroll 8
            for (int c = 0; c < ncars_here; ++c)
                L.scan[(cpb + c) * win_floats + scan_window_first(eighth) + j] = P.ranges[(size_t)(ci0 + c) * P.ranges_stride + eighth + j];
        }
        if ((int)threadIdx.x < ncars_here) L.scan[(cpb + (int)threadIdx.x) * win_floats + win_floats - 1] = P.ranges[(size_t)(ci0 + (int)threadIdx.x) * P.ranges_stride];
    }
    for (int c = wave; c < ncars_here; c += nwaves) {
        const int ci = ci0 + c;
        if (lane < (int)(sizeof(CarCore) / 4))
            reinterpret_cast<uint32_t*>(L.cars + c)[lane] = reinterpret_cast<const uint32_t*>(static_cast<const CarCore*>(&P.cars[ci]))[lane];
        if (lane == 0) L.steps[c] = P.steps[ci / P.cars_per_env];
        wave_lds_sync();
        if (lane == 0 && !frame_write(P, L.veh->v, L.cars + c, L.frame + c, c)) atomicOr(L.pool + 4, 1);
    }
    if (DYN) {                           // the cars' dynamics records (read from the next step barrier on)
        const double* src = dyn_table(scalar_view(Pt)) + (size_t)ci0 * FTGP_DYN_RECORD;       // (the address: from the block in device memory, which the first setter call patched)
        double* dst = reinterpret_cast<double*>(lds + P.lds_bytes);
        for (int i = (int)threadIdx.x; i < ncars_here * FTGP_DYN_RECORD; i += (int)blockDim.x) dst[i] = src[i];
    }
    if (MULTI) {                         // env-mate records of the first frames
        __syncthreads();
        // (a loop: one wave per workgroup -- FTGP_WAVES_PER_BLOCK=1 -- has 64 threads for up to 16 cars x FTGP_PAIR_STRIDE records)
        for (int idx = (int)threadIdx.x; idx < ncars_here * FTGP_PAIR_STRIDE; idx += (int)blockDim.x)
            pair_cull_write(L.frame, L.pairs, idx / FTGP_PAIR_STRIDE, idx % FTGP_PAIR_STRIDE, P.cars_per_env, L.veh->cull_radius, (float)L.veh->v.lidar_ring_radius);
        __syncthreads();
        if (wave == 0) {                 // for the list step 0's sweep draws from: the window-only one unless that step is the launch's last (see the step loop)
            const bool win0 = need_scan && n_steps != 1 && P.win_tasks_per_car != 0;
            mate_masks(L.frame, L.pairs, L.mmask, P.mmask_stride, win0 ? &scalar_view(Pt)->win_group_order[0] : &scalar_view(Pt)->group_order[0], L.ray, P.n_rays,
                       win0 ? P.win_tasks_per_car : P.tasks_per_car, P.cars_per_env, L.veh->cull_radius, P.group_cg, P.group_sg, ncars_here, lane_here(), FTGP_WAVE);
        }
    }
    }
    __syncthreads();

    // One workgroup barrier per step.  Inside a step, concurrently:
    //   waves 0 .. cars-1  K5: driver of one car each on the scan of the PREVIOUS step (the other scan buffer) -> controls;
    //                      the wave whose driver finishes last runs K1 + K3 for all cars (one car per lane) and writes the
    //                      LiDAR frames of the NEXT step into the other frame buffer
    //   every wave         K2: the sweep of THIS step from the current frame buffer (as soon as its driver work is done)
    // The scan a driver sees lags the pose by one step (custom.py:1395-1425), which is what makes this legal: the sweep of
    // step t needs only the pose of step t, and that depends on the controls of step t-1.
    STAMP_DECLARE();
    for (int it = 0; it < n_steps; ++it) {
        STAMP(t0);
        // Each phase of a step fetches what it needs of the parameter block with scalar loads (scalar_view) and sees the LDS arrays
        // through fresh offsets: nothing of this is carried -- spilled -- from step to step or across the other phase.
        const int par = it & 1;
        if (wave < ncars_here) {         // drivers (and, for the wave that delivers last, dynamics)
            const ScalarParams G = scalar_view(Pt);
            const LdsOffsets off = lds_offsets(G);
            const DeviceParams& P = *reinterpret_cast<const DeviceParams*>(lds + off.params);
            const Lds L = lds_view(off, lds);
            const int win_floats = G->win_floats;
            LidarFrame* next_frames = L.frame + (par ^ 1) * cpb;
            float* scan_prev = L.scan + (par ^ 1) * cpb * win_floats;
            // the driver -> dynamics chain is the latency-critical path of a step and a small share of its instructions: let it issue first
            if (FTGP_DIAG_PRIO) __builtin_amdgcn_s_setprio(3);
            for (int c = wave; c < ncars_here; c += nwaves) {
                if constexpr (NET) {      // the launch's driver, or some slot's, is a network: the slot's driver, networks among them
                    const int pol = policy == FTGP_POLICY_PER_CAR ? G->car_policy[c] : policy;
                    if (is_net_policy(pol)) policy_apply_net(net_table(G), pol - FTGP_POLICY_NET0, scan_prev + c * win_floats, G->eighth, L.cars + c,
                                                            [&] { const int cpe = G->cars_per_env, sl = c % cpe; return NetEnv{ L.path, L.cars + (c - sl), (int)sizeof(CarCore), sl, cpe }; },
                                                            [&] { return (ci0 + c) / G->cars_per_env; });
                    else if (policy == FTGP_POLICY_PER_CAR)
                        policy_apply(P, driver_shape(G), pol, scan_prev + c * win_floats, L.cars + c, ci0 + c, L.steps[c], L.list + wave * FTGP_WAVE,
                                     L.cover + (pol == FTGP_POLICY_FAST ? (G->stage_cover >> 2) : 0));
                }
                else if (ROSTER && policy == FTGP_POLICY_PER_CAR) {
                    // the roster's drivers: car slot c of the workgroup has its own (wave-uniform: a scalar load); both cover tables are staged
                    const int pol = G->car_policy[c];
                    policy_apply(P, driver_shape(G), pol, scan_prev + c * win_floats, L.cars + c, ci0 + c, L.steps[c], L.list + wave * FTGP_WAVE,
                                 L.cover + (pol == FTGP_POLICY_FAST ? (G->stage_cover >> 2) : 0));
                }
                else if (policy != FTGP_POLICY_HOST) policy_apply(P, driver_shape(G), policy, scan_prev + c * win_floats, L.cars + c, ci0 + c, L.steps[c], L.list + wave * FTGP_WAVE, L.cover);
                wave_lds_sync();
                // "my controls are in LDS" -> the wave that counts last reads every car's controls: release on this side (the
                // fence of wave_lds_sync() + the RMW), acquire on the reader's (the RMW + the fence below), workgroup scope
                int n = 0;
                if (lane_here() == 0) n = __hip_atomic_fetch_add(L.pool + 2 + par, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
                n = __builtin_amdgcn_readfirstlane(n);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                STAMP(t1); STAMP_ADD(0, t1 - t0);
                if (n == ncars_here - 1) {            // every driver of the workgroup has delivered its controls
                    if (lane_here() == 0) { L.pool[par ^ 1] = 0; L.pool[2 + (par ^ 1)] = 0; }     // the next step's counters (idle during this step)
                    // (the masks of the next step's frames: for the list its sweep draws from, see window_only below)
                    const bool win_next = need_scan && it + 1 != n_steps - 1 && G->win_tasks_per_car != 0;
                    if (FTGP_DIAG_RUN_K1)
                        dynamics_lanes<MULTI, DYN>(P, L, next_frames, L.pairs + (par ^ 1) * cpb * FTGP_PAIR_STRIDE, L.mmask + (par ^ 1) * cpb * G->mmask_stride, &G->group_order[0], win_next,
                                                   L.pool + 4 + (par ^ 1), ncars_here, ci0, DYN ? reinterpret_cast<const double*>(lds + opaque(G->lds_bytes)) : nullptr);
                    STAMP(t2); STAMP_ADD(2, t2 - t1); STAMP_ADD(7, 1);
                }
            }
            if (FTGP_DIAG_PRIO) __builtin_amdgcn_s_setprio(0);
        }
        STAMP(t3);
        if (FTGP_DIAG_RUN_K2) {
            const ScalarParams G = scalar_view(Pt);
            const LdsOffsets off = lds_offsets(G);
            const DeviceParams& P = *reinterpret_cast<const DeviceParams*>(lds + off.params);
            const Lds L = lds_view(off, lds);
            // The ranges of a step inside a launch whose drivers read the scan have one reader: the next step's driver, through the LDS window.
            // Whatever reads the rows in HBM runs after the launch and sees its last step.  So only that step sweeps the whole fan and stores
            // it (FTGP_SCAN_EVERY_STEP: win_tasks_per_car = 0, every step does).  A launch whose drivers do not read the scan keeps the full sweep.
            const bool window_only = need_scan && it != n_steps - 1 && G->win_tasks_per_car != 0;
            if (FAKE) lidar_fake(G, L.frame + par * cpb, L.scan + par * cpb * G->win_floats, L.pool + par, ncars_here, ci0, need_scan, window_only);
            else if (window_only)
                lidar_groups<MULTI, true>(P, G, L, L.frame + par * cpb, L.pairs + par * cpb * FTGP_PAIR_STRIDE, L.mmask + par * cpb * G->mmask_stride, L.scan + par * cpb * G->win_floats,
                                          L.pool + par, ncars_here, ci0, true, second_half STAMP_PASS);
            else
                lidar_groups<MULTI, false>(P, G, L, L.frame + par * cpb, L.pairs + par * cpb * FTGP_PAIR_STRIDE, L.mmask + par * cpb * G->mmask_stride, L.scan + par * cpb * G->win_floats,
                                           L.pool + par, ncars_here, ci0, need_scan, second_half STAMP_PASS);
        }
        STAMP(t4);
        __syncthreads();
        STAMP(t5);
        STAMP_ADD(3, t4 - t3); STAMP_ADD(4, t5 - t4); STAMP_ADD(5, 1); STAMP_ADD(6, t5 - t0);
    }

    STAMP_FLUSH();
    const DeviceParams& P = P0;
    const LdsOffsets off_end = lds_offsets(scalar_view(Pt));
    const Lds L = lds_view(off_end, lds);
    for (int c = wave; c < ncars_here; c += nwaves) {
        const int ci = ci0 + c;
        if (lane_here() < (int)(sizeof(CarCore) / 4))
            reinterpret_cast<uint32_t*>(static_cast<CarCore*>(&P.cars[ci]))[lane_here()] = reinterpret_cast<const uint32_t*>(L.cars + c)[lane_here()];
        if (lane_here() == 0 && ci % P.cars_per_env == 0) P.steps[ci / P.cars_per_env] = L.steps[c];
    }
    if (P.wg_metrics) {                  // the scan windows and the centre line are dead now: the reduction's scratch
        if (metrics_slot & 2) launch_metrics<true>(P, L.cars, L.steps, ncars_here, ci0, nullptr, nullptr, metrics_slot & 1, wave);      // (LDS state records: final since the last step's barrier)
        else {
            __syncthreads();
            launch_metrics<false>(P, L.cars, L.steps, ncars_here, ci0, lds + P.off_scan, reinterpret_cast<double*>(lds + P.off_path), metrics_slot, wave);
        }
    }
    FTGP_DIAG_WG_EXIT();
}

template __global__ void ftgp_step_kernel<false, false, false, false>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, false, false>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, false>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, false>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, true, true, false>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, true, true, false>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, true, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, true, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, false, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, false, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, false, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, false, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, false, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, false, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, true, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, true, false, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, false, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, false, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<false, false, true, true, true, true>(const DeviceParams*, int, int, int);
template __global__ void ftgp_step_kernel<true, false, true, true, true, true>(const DeviceParams*, int, int, int);

// K5 alone: one wave per car evaluates the driver on the scan stored in P.ranges (ftgp_policy_eval).
// env_track: the track of every env, null with one track (a network's frame inputs read the centre-line of the car's track)
__global__ void __launch_bounds__(256) ftgp_policy_kernel(DeviceParams P, int policy, double* __restrict__ ctrl_out, const int32_t* __restrict__ env_track)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ci = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
    if (ci >= P.n_cars) return;
    const int win_floats = P.win_floats;
    CarCore* st = reinterpret_cast<CarCore*>(lds) + wave;
    int* list = reinterpret_cast<int*>(lds + 4 * sizeof(CarCore)) + wave * FTGP_WAVE;
    float* scan = reinterpret_cast<float*>(lds + 4 * sizeof(CarCore) + 4 * FTGP_WAVE * sizeof(int)) + wave * win_floats;
    const float* my_ranges = P.ranges + (size_t)ci * P.ranges_stride;
    if (lane == 0) scan[win_floats - 1] = my_ranges[0];
    for (int j = P.eighth + lane; j < P.n_rays - P.eighth; j += FTGP_WAVE) scan[scan_window_first(P.eighth) + j - P.eighth] = my_ranges[j];
    if (lane < (int)(sizeof(CarCore) / 4))
        reinterpret_cast<uint32_t*>(st)[lane] = reinterpret_cast<const uint32_t*>(static_cast<const CarCore*>(&P.cars[ci]))[lane];
    wave_lds_sync();
    const int pol = policy == FTGP_POLICY_PER_CAR ? P.car_policy[ci % P.cars_per_env] : policy;
    if (is_net_policy(pol))
        policy_apply_net(net_table(&P), pol - FTGP_POLICY_NET0, scan, P.eighth, st,
                         [&] { const int env = ci / P.cars_per_env;
                               return NetEnv{ P.path + (size_t)(env_track ? env_track[env] : 0) * 2 * FTGP_PATH_POINTS, P.cars + (size_t)env * P.cars_per_env,
                                              (int)sizeof(CarState), ci - env * P.cars_per_env, P.cars_per_env }; },
                         [&] { return ci / P.cars_per_env; });
    else policy_apply(P, driver_shape(&P), pol, scan, st, ci, P.steps[ci / P.cars_per_env], list, P.cover_thr + (pol == FTGP_POLICY_FAST ? P.cover_kmax + 1 : 0));
    wave_lds_sync();
    if (lane == 0) {
        P.cars[ci].u_speed = st->u_speed; P.cars[ci].u_steer = st->u_steer; P.cars[ci].last_steer = st->last_steer;
        if (ctrl_out) { ctrl_out[2 * ci] = st->u_speed; ctrl_out[2 * ci + 1] = st->u_steer; }
    }
}

// ftgp_set_net_device: the parameters of a slot from the caller's layout (per layer W[n_out][n_in], then b[n_out]) into the library's
// (NetDev: Wt[n_in][ld], then b[ld]); one thread per parameter, the padding stays the zeros ftgp_set_net wrote.  n = the caller's count.
// ftgp_set_net_population_device: the same for every one of n_members members, n floats apart in src, stride floats apart in dst;
// members blockIdx.y, blockIdx.y + gridDim.y, ... (the host caps the grid's y at FTGP_NET_PARAMS_GRID_Y, n_members is bounded by n_envs alone).
#define FTGP_NET_PARAMS_GRID_Y 1024
__global__ void ftgp_net_params_kernel(NetDev N, const float* __restrict__ src, float* __restrict__ dst, int n, int stride, int n_members)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int at = ftgp_net_library_index(N.n_layers, N.width, i);       // (i < n = the caller's count: never -1)
    for (int m = blockIdx.y; m < n_members; m += gridDim.y) dst[(size_t)m * (size_t)stride + (size_t)at] = src[(size_t)m * (size_t)n + (size_t)i];
}

// ftgp_collect_device, step 1 "Act" (include/ftgp.h "Collected rollouts"): one wave per external car, four per workgroup, as K5 alone.
// The wave stages the rays its network's beams cover and the car's record in LDS, forms the inputs (net_inputs) and writes them down
// -- input i from lane i % 64, n_in consecutive floats per row --, evaluates the layers (net_layers), and lanes 0 and 1 turn the two
// outputs into mean and action with the element operations of ftgp_net.h.  ACT = false: the input half alone (next_inputs).
// (A template, behind the step kernel's instantiations in the file: the code object lays the kernels out in that order, and the
// step kernels stay where they were.)
struct CollectActArgs {
    const float* noise;           // [n_rows][2] or null = zeros
    float* inputs;                // [n_rows][n_in]; the VALUE instantiations take null = not written down
    float* mean;                  // [n_rows][2]; unused, as noise and action, by the ACT = false instantiation
    float* action;                // [n_rows][2]
    float std[2], lo[2], hi[2];
    int32_t slot, n_ext, n_rows, pad;
    int32_t ext_slot[FTGP_PAIR_STRIDE];      // index among the env's external cars -> car slot
    const int32_t* env_track;     // the track of every env; null with one track (frame inputs: the centre-line of the car's track)
};
// VALUE (ftgp_collect_values_device, steps 1' and 3'): the wave keeps a copy of x, evaluates the slot's value net on it -- net_layers on a
// NetDev-shaped record of the value net, one parameter set whatever the slot's population -- and lane 0 writes v.  For a finished car
// too: its policy is not looked at, its value is.  With ACT = false the value is the only evaluation (next_value).  The record and the
// row come behind CollectActArgs in an argument struct of the VALUE instantiations' own: the two instantiations without it take the
// arguments they took and hold the code they held.
struct CollectValueArgs : CollectActArgs {
    const NetDev* vnet;           // the value record of the slot (FtgpEnv::d_vnets + slot)
    float* value;                 // [n_rows]
};
template <bool VALUE> struct CollectArgsOf { typedef CollectActArgs type; };
template <> struct CollectArgsOf<true> { typedef CollectValueArgs type; };
template <bool ACT, bool VALUE = false>
__global__ void __launch_bounds__(256) ftgp_collect_act_kernel(DeviceParams P, typename CollectArgsOf<VALUE>::type C)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
    if (row >= C.n_rows) return;                                 // (whole waves leave: nothing below meets a workgroup barrier)
    const int ci = (row / C.n_ext) * P.cars_per_env + C.ext_slot[row % C.n_ext];
    const ScalarNet N = scalar_net(net_table(&P), C.slot);
    CarCore* st = reinterpret_cast<CarCore*>(lds) + wave;
    // the rays of the beams: [beam_first * pool, (beam_first + n_beams) * pool), inside the car's row by ftgp_set_net's rule; a wave's part of
    // the LDS holds exactly these (the host sizes it: collect_act_lds)
    const int j0 = N->beam_first * N->pool, j1 = j0 + N->n_beams * N->pool;
    float* scan = reinterpret_cast<float*>(lds + 4 * sizeof(CarCore)) + wave * (j1 - j0);
    float* win = scan - j0;                                      // sample j of the car's scan sits at win[j]
    const float* my_ranges = P.ranges + (size_t)ci * P.ranges_stride;
    for (int j = j0 + lane; j < j1; j += FTGP_WAVE) win[j] = my_ranges[j];
    if (lane < (int)(sizeof(CarCore) / 4))
        reinterpret_cast<uint32_t*>(st)[lane] = reinterpret_cast<const uint32_t*>(static_cast<const CarCore*>(&P.cars[ci]))[lane];
    wave_lds_sync();
    float x[4];
    net_inputs(N, win, st, [&] { const int env = row / C.n_ext;
                                 return NetEnv{ P.path + (size_t)(C.env_track ? C.env_track[env] : 0) * 2 * FTGP_PATH_POINTS, P.cars + (size_t)env * P.cars_per_env,
                                                (int)sizeof(CarState), ci - env * P.cars_per_env, P.cars_per_env }; }, x);
    const int n_in = N->width[0];
    if (!VALUE || C.inputs) {                                    // (next_value without next_inputs: x is not written down)
        float* in_row = C.inputs + (size_t)row * n_in;
        #pragma unroll
        for (int r = 0; r < 4; ++r) if (r * FTGP_WAVE + lane < n_in) in_row[r * FTGP_WAVE + lane] = x[r];
    }
    if (!ACT && !VALUE) return;
    if constexpr (VALUE) {
        const ScalarNet V = scalar_net(C.vnet, 0);
        float xv[4] = { x[0], x[1], x[2], x[3] };
        net_layers(V, [] { return 0; }, xv);                     // (a value record has no env_member: the env is never asked for)
        if (lane == 0) C.value[row] = ftgp_net_value(xv[0], V->out_scale[0], V->out_offset[0]);
        if (!ACT) return;
    }
    const int k = lane & 1;
    float m = 0.0f, a = 0.0f;
    if (!sgpr(st->finished)) {                                   // a finished car: (0, 0) before the network is looked at
        net_layers(N, [&] { return row / C.n_ext; }, x);
        const float nz = C.noise ? C.noise[(size_t)row * 2 + k] : 0.0f;
        m = ftgp_net_mean(x[0], k ? N->out_scale[1] : N->out_scale[0], k ? N->out_offset[1] : N->out_offset[0]);
        a = ftgp_net_clip(ftgp_net_noisy(m, k ? C.std[1] : C.std[0], nz), k ? C.lo[1] : C.lo[0], k ? C.hi[1] : C.hi[0]);
        const bool both = (__ballot(ftgp_net_finite(a)) & 3ull) == 3ull;
        a = ftgp_net_guarded(a, both);
    }
    if (lane < 2) { C.mean[(size_t)row * 2 + lane] = m; C.action[(size_t)row * 2 + lane] = a; }
}

template __global__ void ftgp_collect_act_kernel<true>(DeviceParams, CollectActArgs);
template __global__ void ftgp_collect_act_kernel<false>(DeviceParams, CollectActArgs);

// ftgp_set_net_population_device: the env-to-member map from the caller's buffer; an entry outside [0, n_members) cannot be refused without
// a synchronisation and becomes member 0, so that no car reads parameters outside the population's buffer
__global__ void ftgp_net_map_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int n_envs, int n_members)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_envs) return;
    const int32_t m = src[e];
    dst[e] = (m >= 0 && m < n_members) ? m : 0;
}

// =============================================================================================
// K4: reset / spawn (custom.py:1089-1128, 1232-1245, 81-87), one car per lane; then K3 at the spawn pose.
// =============================================================================================
// Multi-track handles: the track of every env (env_track, [n_envs]; null with one track).  Track t's centre-line and spawn table sit
// t tables behind track 0's (P.path, P.spawn).
__device__ __forceinline__ int env_track_of(const int32_t* __restrict__ env_track, int env) { return env_track ? env_track[env] : 0; }

// path: the centre-line of the car's track
__device__ __forceinline__ void progress_lane(const DeviceParams& P, const double* __restrict__ path, CarCore& s, int64_t steps, double* __restrict__ times)
{
    double best = 0.0; int closest = 0;
    for (int i = 0; i < FTGP_PATH_POINTS; ++i) {
        const double dx = path[2 * i] - s.x, dy = path[2 * i + 1] - s.y;
        const double d = dx * dx + dy * dy;
        if (i == 0 || d < best) { best = d; closest = i; }
    }
    Race r; race_load(r, &s);
    progress_update(P, r, steps, closest, best, times, &s.start);
    race_store(r, &s);
}

// the spawn state of car ci (car `car` of env `env`, on track trk) with a cleared race state, before K3 has seen the spawn pose.
// With a spawn rule (R set: the rule in device memory; ftgp_set_spawn_rule) the pose is that episode's draw of ftgp_spawn.h and the progress offset the
// nearest centre-line point of that pose; without one, spawn_mode 0 / 1 as ever.
__device__ __forceinline__ void spawn_state(const DeviceParams& P, const FtgpSpawnDev* __restrict__ R, int64_t episode, int ci, int env, int car, int trk, CarCore& s)
{
    const double* spawn = P.spawn + (size_t)trk * 4 * FTGP_PATH_POINTS;
    memset(&s, 0, sizeof s);
    if (R) {
        FtgpSpawnPose o;
        ftgp_spawn_draw(P.seed, (uint64_t)(P.env_base + env), (uint64_t)episode, P.cars_per_env, car, R->start + (size_t)trk * FTGP_PATH_POINTS, R->n_start[trk],
                        R->clear + (size_t)trk * 2 * FTGP_PATH_POINTS, spawn, R->margin, R->lateral_frac, R->yaw_tan, R->shuffle_grid, o);
        s.offset = o.offset;
        s.good_start = 1;
        s.x = o.x; s.y = o.y; s.qw = o.qw; s.qz = o.qz;
        return;
    }
    const int p = (P.spawn_mode == 0) ? (car + 5) * 2 : (int)((10 + 7 * (long)(P.env_base + env) + 2 * car) % 98);   // custom.py:1112
    s.offset = p;
    s.good_start = 1;
    s.x = spawn[4 * p]; s.y = spawn[4 * p + 1];
    double qw = spawn[4 * p + 2], qz = spawn[4 * p + 3];
    if (P.spawn_mode == 1) {
        const uint64_t h = splitmix64(P.seed ^ (0xA0761D6478BD642Full + (uint64_t)((long)P.env_base * P.cars_per_env + ci)));
        const double j = 0.2 * u01(h) - 0.1;
        const double cj = spec_cos(0.5 * j), sj = spec_sin(0.5 * j);
        const double nw = qw * cj - qz * sj, nz = qz * cj + qw * sj;
        const double n = sqrt(nw * nw + nz * nz);
        qw = nw / n; qz = nz / n;
    }
    s.qw = qw; s.qz = qz;
}

// car ci back at its spawn pose with a cleared race state; car 0 of the env also zeroes the env's steps (ftgp_reset_kernel and both finish
// kernels).  episode: the env's episode counter as every car of the env read it before anyone advances it (spawn rule only).  The record is
// reset where it lies, without a copy on the lane's stack -- K3 reaches start / finish_step through a pointer, which would keep such a copy
// in scratch memory
__device__ __forceinline__ void reset_car(const DeviceParams& P, int ci, const int32_t* __restrict__ env_track, const FtgpSpawnDev* __restrict__ R, int64_t episode)
{
    const int env = ci / P.cars_per_env, car = ci % P.cars_per_env;
    const int trk = env_track_of(env_track, env);
    CarCore& s = P.cars[ci];
    spawn_state(P, R, episode, ci, env, car, trk, s);
    if (car == 0) P.steps[env] = 0;
    for (int k = 0; k < FTGP_MAX_LAP_TIMES; ++k) P.cars[ci].times[k] = 0.0;
    progress_lane(P, P.path + (size_t)trk * 2 * FTGP_PATH_POINTS, s, 0, P.cars[ci].times);
}

// With a spawn rule the cars of an env -- lanes of different waves, even of different workgroups -- all spawn with the env's episode
// counter as it stands: nobody advances it here, ftgp_episodes_kernel does in a launch of its own behind this one.
__global__ void ftgp_reset_kernel(DeviceParams P, const uint8_t* __restrict__ env_mask, const int32_t* __restrict__ env_track, const FtgpSpawnDev* __restrict__ R)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    const int env = ci / P.cars_per_env;
    if (env_mask && !env_mask[env]) return;
    reset_car(P, ci, env_track, R, R ? R->episodes[env] : 0);
}

// spawn rule: the episode counters of the envs just reset, one env per lane
__global__ void ftgp_episodes_kernel(int n_envs, const uint8_t* __restrict__ env_mask, int64_t* __restrict__ episodes)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n_envs) return;
    if (env_mask && !env_mask[env]) return;
    episodes[env] += 1;
}

// sensordata = 0 after mj_resetData (custom.py:1092): coalesced zero fill of the reset envs' scans
__global__ void ftgp_zero_ranges_kernel(DeviceParams P, const uint8_t* __restrict__ env_mask)
{
    const int ci = blockIdx.x;
    if (env_mask && !env_mask[ci / P.cars_per_env]) return;
    float* r = P.ranges + (size_t)ci * P.ranges_stride;
    for (int j = threadIdx.x; j < P.ranges_stride; j += blockDim.x) r[j] = 0.0f;
}

__global__ void ftgp_progress_kernel(DeviceParams P, const int32_t* __restrict__ env_track)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    CarCore s = static_cast<const CarCore&>(P.cars[ci]);
    const int env = ci / P.cars_per_env;
    progress_lane(P, P.path + (size_t)env_track_of(env_track, env) * 2 * FTGP_PATH_POINTS, s, P.steps[env], P.cars[ci].times);
    static_cast<CarCore&>(P.cars[ci]) = s;
}

__global__ void ftgp_set_ctrl_kernel(DeviceParams P, const double* __restrict__ ctrl, const uint8_t* __restrict__ mask)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    if (mask && !mask[ci]) return;
    P.cars[ci].u_speed = ctrl[2 * ci];
    P.cars[ci].u_steer = ctrl[2 * ci + 1];
}

// ftgp_set_dynamics / ftgp_set_dynamics_device: one car per thread writes its dynamics record -- at `init` the handle's own row, then, for
// a car of a masked env, the caller's row if it is valid (every entry finite, mass > 0, izz > 0, entries 2-7 >= 0); an invalid row leaves
// the record as it is and counts.  A second mask, if given, is OR-ed with the first (ftgp_collect_device).  The wheel loads are plan()'s expressions on the row's mass (binary64, one rounding per operation).
__device__ __forceinline__ void dyn_record_write(double* rec, const double* row, const DynArgs& A)
{
    for (int k = 0; k < FTGP_DYN_DOUBLES; ++k) rec[k] = row[k];
    const double wtot = row[kDynMass] * A.gravity;
    for (int r = 0; r < 4; ++r) {
        const double w = wtot * A.load_k[r];
        rec[kDynWheelLoad + r] = A.load_half[r] ? 0.5 * w : w;
    }
}

__global__ void ftgp_dynamics_kernel(DeviceParams P, DynArgs A)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_cars) return;
    double* rec = dyn_table(&P) + (size_t)i * FTGP_DYN_RECORD;
    if (A.init) dyn_record_write(rec, A.base, A);
    if (!A.rows || (A.env_mask && !(A.env_mask[i / P.cars_per_env] | (A.env_mask_or ? A.env_mask_or[i / P.cars_per_env] : 0)))) return;
    double row[FTGP_DYN_DOUBLES];
    bool ok = true;
    for (int k = 0; k < FTGP_DYN_DOUBLES; ++k) {
        row[k] = A.rows[(size_t)i * FTGP_DYN_DOUBLES + k];
        ok = ok && row[k] >= 0.0 && row[k] < INFINITY;            // (false for a NaN)
    }
    ok = ok && row[kDynMass] > 0.0 && row[kDynIzz] > 0.0;
    if (ok) dyn_record_write(rec, row, A);
    else atomicAdd(dyn_rejected(&P), 1ull);
}

__global__ void ftgp_set_pose_kernel(DeviceParams P, const double* __restrict__ pose)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    const double* o = pose + (size_t)ci * FTGP_POSE_DOUBLES;
    const double n = sqrt(o[3] * o[3] + o[6] * o[6]);
    CarState& s = P.cars[ci];
    s.x = o[0]; s.y = o[1]; s.qw = o[3] / n; s.qz = o[6] / n; s.vx = o[7]; s.vy = o[8]; s.wz = o[12];
}

// =============================================================================================
// Device I/O (ftgp_step_device): the caller's actions in, observations / rewards / episode ends out, all in device memory.
// A call is: ftgp_io_ingest_kernel -> ftgp_step_kernel<.., ROSTER> (action_repeat steps) -> ftgp_io_finish_kernel; with contacts on,
// ftgp_io_contact_kernel runs between the steps and the finish kernel; with the frame on, so does ftgp_io_frame_kernel, and with the dense
// reward it also runs behind the ingest kernel, at the pose the call begins with.  With rivals on ftgp_io_rival_kernel follows the frame
// kernel behind the steps (which runs for the rivals' sake if the frame is off), and with the place reward both run behind the ingest kernel too.
// =============================================================================================
struct DeviceIoArgs {
    const float* action;          // [n_envs][n_ext][2] (speed, steering_angle)
    float* obs;                   // [n_envs][n_ext][n_rays]
    float* reward;                // [n_envs][n_ext]
    uint8_t* terminated;          // [n_envs]
    uint8_t* truncated;           // [n_envs]
    float* final_obs;             // [n_envs][n_ext][n_rays] or null
    int32_t* prev_abs;            // [n_cars] absolute_completion before the call's steps
    int64_t max_episode_steps;    // <= 0: never truncate
    int32_t n_ext, auto_reset;
    int32_t vec4;                 // n_rays % 4 == 0 and obs / final_obs 16-byte aligned: rows move as float4
    int32_t ext_index[FTGP_PAIR_STRIDE];   // car slot -> its index among the env's external cars, -1 = a bundled driver
    const int32_t* env_track;     // multi-track handles: the track of every env (reset_car); null with one track
};

// custom.py:132-143, as ftgp_get_progress column 3 reports it
__device__ __forceinline__ int32_t absolute_completion(const CarCore& a)
{
    return a.laps * 100 + (a.good_start ? a.completion : -(100 - a.completion));
}

// One car per lane: external cars take the caller's action -- (0, 0) once finished, the null driver of custom.py:1441-1447 --
// and every car's absolute_completion is kept for the reward.
__global__ void ftgp_io_ingest_kernel(DeviceParams P, DeviceIoArgs A)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    CarState& s = P.cars[ci];
    A.prev_abs[ci] = absolute_completion(s);
    const int k = A.ext_index[ci % P.cars_per_env];
    if (k < 0) return;
    const float* a = A.action + 2 * ((size_t)(ci / P.cars_per_env) * A.n_ext + k);
    const bool fin = s.finished != 0;
    s.u_speed = fin ? 0.0 : (double)a[0];
    s.u_steer = fin ? 0.0 : (double)a[1];
}

// One workgroup per env, after the steps: rewards, episode ends, and the observations.  An env that ended with auto_reset on
// hands its scans to final_obs, gets obs rows of zeros and is reset exactly as ftgp_reset resets it (reset_car, ranges 0).
#define FTGP_IO_THREADS 256
__global__ void __launch_bounds__(FTGP_IO_THREADS) ftgp_io_finish_kernel(DeviceParams P, DeviceIoArgs A, const FtgpSpawnDev* __restrict__ rule)
{
    __shared__ int ended;
    const int env = blockIdx.x, cpe = P.cars_per_env, ci0 = env * cpe, t = threadIdx.x;
    const int64_t episode = rule ? rule->episodes[env] : 0;      // spawn rule: read by every lane before the barriers, advanced behind them
    if (t == 0) {
        bool all_finished = true;
        for (int c = 0; c < cpe; ++c)
            if (A.ext_index[c] >= 0 && !P.cars[ci0 + c].finished) all_finished = false;
        const bool trunc = !all_finished && A.max_episode_steps > 0 && P.steps[env] >= A.max_episode_steps;
        A.terminated[env] = all_finished ? 1 : 0;
        A.truncated[env] = trunc ? 1 : 0;
        ended = (all_finished || trunc) ? 1 : 0;
    }
    if (t < cpe && A.ext_index[t] >= 0)
        A.reward[(size_t)env * A.n_ext + A.ext_index[t]] = (float)(absolute_completion(P.cars[ci0 + t]) - A.prev_abs[ci0 + t]);
    __syncthreads();
    const bool reset = A.auto_reset && ended;
    const int R = P.n_rays;
    for (int c = 0; c < cpe; ++c) {
        const int k = A.ext_index[c];
        float* src = P.ranges + (size_t)(ci0 + c) * P.ranges_stride;
        if (k >= 0) {
            const size_t row = ((size_t)env * A.n_ext + k) * R;
            float* obs = A.obs + row;
            float* fin = A.final_obs ? A.final_obs + row : nullptr;
            if (A.vec4) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int j = t; j < R / 4; j += FTGP_IO_THREADS) {
                    const float4 v = reinterpret_cast<const float4*>(src)[j];
                    if (!reset) { reinterpret_cast<float4*>(obs)[j] = v; continue; }
                    if (fin) reinterpret_cast<float4*>(fin)[j] = v;
                    reinterpret_cast<float4*>(obs)[j] = z;
                }
            } else {
                for (int j = t; j < R; j += FTGP_IO_THREADS) {
                    const float v = src[j];
                    if (!reset) { obs[j] = v; continue; }
                    if (fin) fin[j] = v;
                    obs[j] = 0.0f;
                }
            }
        }
        __syncthreads();      // the row has been read before it is zeroed
        if (reset) for (int j = t; j < P.ranges_stride; j += FTGP_IO_THREADS) src[j] = 0.0f;
    }
    if (reset && t < cpe) reset_car(P, ci0 + t, A.env_track, rule, episode);      // (the records were read before the first barrier)
    if (reset && t == 0 && rule) rule->episodes[env] = episode + 1;
}

// ---------------------------------------------------------------------------------------------
// Device I/O with signals (ftgp_device_io_signals / ftgp_step_device_ex): the same call with ftgp_io_finish_signals_kernel in the
// place of ftgp_io_finish_kernel -- pooled and scaled scans, a state row per external car, off-track episode ends and penalty.
// ---------------------------------------------------------------------------------------------
#define FTGP_SIG_STAGE_FLOATS 4096      // LDS stage of the pooled scan: a chunk is (FTGP_SIG_STAGE_FLOATS / pool) & ~3 beams, whatever n_rays
#define FTGP_SIG_WAVE_POOL 64           // from this pool on a wave takes a whole beam
enum { FTGP_SIG_PATH_REGS = 0, FTGP_SIG_PATH_STAGE = 1, FTGP_SIG_PATH_WAVE = 2 };
struct DeviceSignalArgs {
    float* state;                 // [n_envs][n_ext][FTGP_STATE_FLOATS] or null
    float* final_state;           // [n_envs][n_ext][FTGP_STATE_FLOATS] or null
    int32_t pool, n_beams;        // rays per beam, beams per row (n_rays / pool)
    int32_t path;                 // FTGP_SIG_PATH_*: how a row is pooled (pooled_row)
    int32_t chunk_beams;          // FTGP_SIG_PATH_STAGE: beams per staged chunk, a multiple of 4
    int32_t vec_in;               // n_rays % 4 == 0: rows are read as float4 (they start on 128-byte boundaries)
    int32_t vec_out;              // n_beams % 4 == 0 and obs / final_obs 16-byte aligned: beams are written as float4
    int32_t clip;                 // scan_max_range > 0
    int32_t terminate_off_track;
    float limit;                  // what a ray without a hit counts as in the minimum: scan_max_range, +inf for raw ranges
    float inv_max_range;          // 1.0f / scan_max_range, divided once on the host
    float penalty;
    // contacts (ftgp_device_io_contacts): filled in per call
    const float* contact_rows;    // [n_cars][FTGP_CONTACT_FLOATS] this call's rows (ftgp_io_contact_kernel), null = contacts are off
    float* contact;               // [n_envs][n_ext][FTGP_CONTACT_FLOATS] or null
    float* final_contact;         // [n_envs][n_ext][FTGP_CONTACT_FLOATS] or null
    int32_t terminate_on_wall, terminate_on_car;
    float wall_penalty, car_penalty;
    // track frame (ftgp_device_io_frame): filled in per call
    const float* frame_rows;      // [n_cars][frame_width] this call's rows (ftgp_io_frame_kernel), null = the frame is off
    float* frame;                 // [n_envs][n_ext][frame_width] or null
    float* final_frame;           // [n_envs][n_ext][frame_width] or null
    const double* frame_s0;       // [n_cars] s at the pose the call began with; null = the integer reward
    const double* frame_s1;       // [n_cars] s at the pose after the steps
    const int32_t* frame_flag0;   // [n_cars] FTGP_FRAME_OFF | FTGP_FRAME_FINISHED when the call began
    const int32_t* frame_flag1;   // [n_cars] ... after the steps
    int32_t frame_ahead, frame_stride;
    // rivals (ftgp_device_io_rivals): filled in per call
    const float* rival_rows;      // [n_cars][rival_width] this call's rows (ftgp_io_rival_kernel), null = rivals are off
    float* rival;                 // [n_envs][n_ext][rival_width] or null
    float* final_rival;           // [n_envs][n_ext][rival_width] or null
    const int32_t* place0;        // [n_cars] the place when the call began, negative for a car that had finished; null = no place reward
    int32_t rival_n;              // mate slots per row
    float place_weight;
};

// a range as it enters the minimum: no hit (< 0) = the limit, a hit = min(r, limit)
__device__ __forceinline__ float sig_ray(float r, float limit) { return r < 0.0f ? limit : fminf(r, limit); }
__device__ __forceinline__ float4 sig_ray4(float4 v, float limit) { return make_float4(sig_ray(v.x, limit), sig_ray(v.y, limit), sig_ray(v.z, limit), sig_ray(v.w, limit)); }
// the minimum as it is written: scaled with one multiplication, or raw with -1 for a beam without a hit
__device__ __forceinline__ float sig_beam(float m, const DeviceSignalArgs& S) { return S.clip ? m * S.inv_max_range : (m == INFINITY ? -1.0f : m); }

// One pooled row by the whole workgroup: src = n_rays ranges (read once, a wave's loads contiguous), out = n_beams floats.
//   REGS   pool 1, 2 or 4, n_rays % 4 == 0 and obs / final_obs 16-byte aligned: a lane's float4 holds whole beams, the minimum never
//          leaves its registers, and the lane writes them as one float4 / float2 / float
//   STAGE  pool < 64: chunks of chunk_beams beams go through LDS as they enter the minimum (float4 in, float4 stage); then one beam per
//          lane, a lane reading its pool consecutive floats (stride pool dwords over the banks: free of conflicts for an odd pool, 2-way
//          for pool 10), and four neighbouring lanes' beams leave as one float4
//   WAVE   pool >= 64: a wave per beam, its lanes striding over the beam, the minimum folded with five shuffles
// No barrier is left pending: a caller may overwrite src after its own barrier.
__device__ __forceinline__ void pooled_row(const float* __restrict__ src, float* __restrict__ out, int R, const DeviceSignalArgs& S, float* stage)
{
    const int t = threadIdx.x, pool = S.pool, NB = S.n_beams;
    const float limit = S.limit;
    if (S.path == FTGP_SIG_PATH_REGS) {
        for (int j = t; j < R / 4; j += FTGP_IO_THREADS) {
            const float4 v = sig_ray4(reinterpret_cast<const float4*>(src)[j], limit);
            if (pool == 1) {
                reinterpret_cast<float4*>(out)[j] = make_float4(sig_beam(v.x, S), sig_beam(v.y, S), sig_beam(v.z, S), sig_beam(v.w, S));
            } else if (pool == 2) {
                reinterpret_cast<float2*>(out)[j] = make_float2(sig_beam(fminf(v.x, v.y), S), sig_beam(fminf(v.z, v.w), S));
            } else {
                out[j] = sig_beam(fminf(fminf(v.x, v.y), fminf(v.z, v.w)), S);
            }
        }
        return;
    }
    if (S.path == FTGP_SIG_PATH_WAVE) {
        const int lane = t & (FTGP_WAVE - 1);
        for (int b = t / FTGP_WAVE; b < NB; b += FTGP_IO_THREADS / FTGP_WAVE) {
            const float* beam = src + (size_t)b * pool;
            float m = limit;
            for (int k = lane; k < pool; k += FTGP_WAVE) m = fminf(m, sig_ray(beam[k], limit));
            for (int d = FTGP_WAVE / 2; d > 0; d >>= 1) m = fminf(m, __shfl_xor(m, d, FTGP_WAVE));
            if (lane == 0) out[b] = sig_beam(m, S);
        }
        return;
    }
    const int CB = S.chunk_beams;
    for (int b0 = 0; b0 < NB; b0 += CB) {
        const int nb = min(CB, NB - b0), n = nb * pool;
        const float* chunk = src + (size_t)b0 * pool;          // (CB % 4 == 0: a chunk starts on a 16-byte boundary)
        if (S.vec_in) {
            for (int j = t; j < n / 4; j += FTGP_IO_THREADS) reinterpret_cast<float4*>(stage)[j] = sig_ray4(reinterpret_cast<const float4*>(chunk)[j], limit);
        } else {
            for (int j = t; j < n; j += FTGP_IO_THREADS) stage[j] = sig_ray(chunk[j], limit);
        }
        __syncthreads();
        for (int b = t; b < ((nb + FTGP_WAVE - 1) & ~(FTGP_WAVE - 1)); b += FTGP_IO_THREADS) {      // whole waves: the shuffles below need every lane
            float m = limit;
            if (b < nb) for (int k = 0; k < pool; ++k) m = fminf(m, stage[b * pool + k]);
            const float v = sig_beam(m, S);
            if (S.vec_out) {          // nb % 4 == 0 then, and b % 4 == lane % 4
                const float v1 = __shfl_down(v, 1, FTGP_WAVE), v2 = __shfl_down(v, 2, FTGP_WAVE), v3 = __shfl_down(v, 3, FTGP_WAVE);
                if ((b & 3) == 0 && b < nb) reinterpret_cast<float4*>(out + b0)[b / 4] = make_float4(v, v1, v2, v3);
            } else if (b < nb) out[b0 + b] = v;
        }
        __syncthreads();      // the stage is free again
    }
}

// the state row of ftgp_step_device_ex / ftgp_state_device (include/ftgp.h): every entry binary64, rounded once
__device__ __forceinline__ void state_row(const CarCore& a, float* __restrict__ o)
{
    const double c = a.qw * a.qw - a.qz * a.qz, s = 2.0 * (a.qw * a.qz);
    const int lc = a.good_start ? a.completion : -(100 - a.completion);         // custom.py:132-140
    o[0] = (float)(a.vx * c + a.vy * s);
    o[1] = (float)(a.vy * c - a.vx * s);
    o[2] = (float)a.wz;
    o[3] = (float)a.u_speed;
    o[4] = (float)a.u_steer;
    o[5] = (float)sqrt(a.dist2);
    o[6] = (float)((double)lc / 100.0);
    o[7] = a.off_track ? 1.0f : 0.0f;
}

// ftgp_state_device: one car per lane
__global__ void ftgp_io_state_kernel(DeviceParams P, DeviceIoArgs A, float* __restrict__ state)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    const int k = A.ext_index[ci % P.cars_per_env];
    if (k < 0) return;
    state_row(P.cars[ci], state + ((size_t)(ci / P.cars_per_env) * A.n_ext + k) * FTGP_STATE_FLOATS);
}

// ---------------------------------------------------------------------------------------------
// Contacts (ftgp_device_io_contacts / ftgp_step_device_contacts / ftgp_contacts_device / ftgp_get_contacts): the contact row of
// include/ftgp.h, from the geometry K1's penalty forces use -- wall_search as K1 calls it, the circle pairs as car_contact_mate forms them.
// ---------------------------------------------------------------------------------------------
struct DeviceContactArgs {
    const unsigned char* blocks;          // the handle's parameter blocks in device memory: track t's DeviceParams at block_off[t]
    const int32_t* env_track;             // the track of every env; null with one track
    float* rows;                          // [n_cars][FTGP_CONTACT_FLOATS]: every car's row, or null
    float* ext_out;                       // [n_envs][n_ext][FTGP_CONTACT_FLOATS]: the external cars' rows, or null
    int32_t n_ext, pad;
    int32_t ext_index[FTGP_PAIR_STRIDE];  // as DeviceIoArgs (read with ext_out only)
    uint32_t block_off[FTGP_MAX_TRACKS];
};

// Sixteen lanes per car, one DPP row: lanes 0..6 take one wall circle each (three chassis circles, the four softeners with bubble_wrap),
// lanes 8..15 take car slot lane - 8 of the env as mate, all nine circle pairs.  Maxima and counts are folded inside each half of the row
// with three shuffles, and lane 0 fetches the mates' half with a fourth.  No LDS, no atomics; a wave holds four cars, a workgroup sixteen.
#define FTGP_CONTACT_LANES 16
#define FTGP_CONTACT_THREADS 256
__global__ void __launch_bounds__(FTGP_CONTACT_THREADS) ftgp_io_contact_kernel(DeviceParams P, DeviceContactArgs C)
{
    // (the car from the block's first car, not from a global lane number: that one would pass 2^31 at 134 M cars)
    const int ci = blockIdx.x * (FTGP_CONTACT_THREADS / FTGP_CONTACT_LANES) + threadIdx.x / FTGP_CONTACT_LANES, l = threadIdx.x % FTGP_CONTACT_LANES;
    const bool live = ci < P.n_cars;
    const int cpe = P.cars_per_env;
    const int env = live ? ci / cpe : 0, slot = live ? ci - env * cpe : 0;
    double pen = 0.0;
    int hit = 0;
    if (live && !P.cars[ci].finished) {          // a finished car collides with nothing (custom.py:1452-1457)
        const CarCore* me = P.cars + ci;
        const FtgpVehicle& v = P.veh;
        if (l < 8) {
            if (l < (P.bubble_wrap ? 7 : 3)) {
                const DeviceParams& Q = *reinterpret_cast<const DeviceParams*>(C.blocks + C.block_off[env_track_of(C.env_track, env)]);
                const bool softener = l >= 3;
                const int k = softener ? l - 3 : l;
                const double qw = me->qw, qz = me->qz;
                const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
                const double rxw = softener ? ch * v.wheel_x[k] - sh * v.wheel_y[k] : ch * v.contact_x[k];
                const double ryw = softener ? sh * v.wheel_x[k] + ch * v.wheel_y[k] : sh * v.contact_x[k];
                const double px = me->x + rxw, py = me->y + ryw;
                const WallHit h = wall_search(Q, Q.bits, Q.nearbits, px, py, softener ? v.softener_radius : v.contact_radius);
                if (h.found) { pen = h.pen; hit = 1; }
            }
        } else {
            const int k = l - 8;
            const CarCore* b = P.cars + (ci - slot + (k < cpe ? k : slot));
            if (k < cpe && k != slot && !b->finished) {
                const double r2 = 2.0 * v.contact_radius;
                const double qw = me->qw, qz = me->qz;
                const double ch = 1.0 - 2.0 * (qz * qz), sh = 2.0 * (qw * qz);
                const double bqw = b->qw, bqz = b->qz;
                const double cb = 1.0 - 2.0 * (bqz * bqz), sb = 2.0 * (bqw * bqz);
                #pragma unroll
                for (int ij = 0; ij < 9; ++ij) {
                    const int i = ij / 3, j = ij - 3 * i;
                    const double rxw = ch * v.contact_x[i], ryw = sh * v.contact_x[i];
                    const double sxw = cb * v.contact_x[j], syw = sb * v.contact_x[j];
                    const double px = me->x + rxw, py = me->y + ryw;
                    const double qx = b->x + sxw, qy = b->y + syw;
                    const double ex = px - qx, ey = py - qy;
                    const double d2 = ex * ex + ey * ey;
                    if (d2 >= r2 * r2 || d2 <= 0.0) continue;
                    const double overlap = r2 - sqrt(d2);
                    if (!hit || overlap > pen) pen = overlap;
                    hit = 1;
                }
            }
        }
    }
    // every lane of the wave is here: the halves of a row fold on their own (xor 1, 2, 4 stay inside eight lanes)
    for (int d = 1; d < 8; d <<= 1) {
        const double o = shfl_xor_f64(pen, d);
        pen = o > pen ? o : pen;
        hit += __shfl_xor(hit, d, FTGP_WAVE);
    }
    const double car_pen = shfl_xor_f64(pen, 8);
    const int car_hit = __shfl_xor(hit, 8, FTGP_WAVE);
    if (!live || l != 0) return;
    const float4 row = make_float4((float)pen, (float)car_pen, (float)hit, (float)car_hit);
    if (C.rows) reinterpret_cast<float4*>(C.rows)[ci] = row;
    if (C.ext_out) {
        const int k = C.ext_index[slot];
        if (k >= 0) {
            float* o = C.ext_out + ((size_t)env * C.n_ext + k) * FTGP_CONTACT_FLOATS;
            o[0] = row.x; o[1] = row.y; o[2] = row.z; o[3] = row.w;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Track frame (ftgp_device_io_frame / ftgp_step_device_frame / ftgp_frame_device / ftgp_get_frames): the frame row of include/ftgp.h --
// the pose projected on the env's centre-line, the track's tangent in the body frame, the lap position, look-ahead points.
// ---------------------------------------------------------------------------------------------
#define FTGP_FRAME_OFF 1                  // flag bits kept per car beside s: d_c > 1.0 at the pose; the car had finished
#define FTGP_FRAME_FINISHED 2
struct DeviceFrameArgs {
    const int32_t* env_track;             // the track of every env; null with one track
    float* rows;                          // [n_cars][FTGP_FRAME_FIXED + 2 * n_ahead]: every car's row, or null
    float* ext_out;                       // [n_envs][n_ext][FTGP_FRAME_FIXED + 2 * n_ahead]: the external cars' rows, or null
    double* s_out;                        // [n_cars]: the unrounded s, or null
    int32_t* flag_out;                    // [n_cars]: FTGP_FRAME_OFF | FTGP_FRAME_FINISHED, or null
    int32_t* c_out;                       // [n_cars]: the nearest point c of step 1 (the rival rows' race progress), or null
    int32_t n_ext, n_ahead, stride, pad;
    int32_t ext_index[FTGP_PAIR_STRIDE];  // as DeviceIoArgs (read with ext_out only)
};

// steps 1 - 6, element by element: ftgp_frame.h (frame_dist2, frame_nearer, frame_segment, frame_fixed, frame_ahead)

// The whole row by one lane (ftgp_io_finish_signals_kernel, the spawn pose of an env it has just reset): the operations of
// ftgp_io_frame_kernel on the same values, the search as the progress block runs it (frame_row).
__device__ __forceinline__ void frame_row_lane(const double* __restrict__ path, const CarCore& a, int n_ahead, int stride, float* __restrict__ o)
{
    frame_row(path, a.x, a.y, a.qw, a.qz, n_ahead, stride, o);
}

// Sixteen lanes per car, one DPP row; a wave holds four cars, a workgroup sixteen.  Lane l walks points l, l + 16, ... and keeps its
// first minimum; the row folds the pair (d, index) with xor-shuffles 1, 2, 4, 8 -- the smaller d wins, on equal d the smaller index, so
// every lane ends with the progress block's first minimum.  (A NaN never wins.  With a NaN pose every d is NaN and each lane keeps its
// own (NaN, l): lane 0 has c = 0 as the progress block does, the other lanes of the row disagree with it, every index stays in 0 .. 99
// and every entry of the row is NaN whichever segment a lane took.)  Lanes 0 and 1 project
// on segment B = c -> c + 1 and A = c - 1 -> c, one shuffle hands A's g2 to lane 0, which takes A only if it is strictly nearer and
// writes the fixed entries, s and the flags; lanes 0 .. n_ahead - 1 write one look-ahead pair each.  No LDS, no atomics.
#define FTGP_FRAME_LANES 16
#define FTGP_FRAME_THREADS 256
__global__ void __launch_bounds__(FTGP_FRAME_THREADS) ftgp_io_frame_kernel(DeviceParams P, DeviceFrameArgs F)
{
    // (the car from the block's first car, not from a global lane number: that one would pass 2^31 at 134 M cars)
    const int ci = blockIdx.x * (FTGP_FRAME_THREADS / FTGP_FRAME_LANES) + threadIdx.x / FTGP_FRAME_LANES, l = threadIdx.x % FTGP_FRAME_LANES;
    const bool live = ci < P.n_cars;
    const int cpe = P.cars_per_env;
    const int env = live ? ci / cpe : 0, slot = live ? ci - env * cpe : 0;
    const double* path = P.path + (size_t)env_track_of(F.env_track, env) * 2 * FTGP_PATH_POINTS;
    double x = 0.0, y = 0.0, qw = 1.0, qz = 0.0;
    int fin = 0;
    double best = INFINITY; int idx = l;      // a lane past n_cars takes part in the shuffles with these
    if (live) {
        const CarCore* me = P.cars + ci;
        x = me->x; y = me->y; qw = me->qw; qz = me->qz; fin = me->finished;
        #pragma unroll 1
        for (int i = l; i < FTGP_PATH_POINTS; i += FTGP_FRAME_LANES) {
            const double dx = path[2 * i] - x, dy = path[2 * i + 1] - y;
            const double d = dx * dx + dy * dy;
            if (i == l || d < best) { best = d; idx = i; }
        }
    }
    // every lane of the wave is here: xor 1, 2, 4, 8 stay inside the row of sixteen
    for (int m = 1; m < FTGP_FRAME_LANES; m <<= 1) {
        const double od = shfl_xor_f64(best, m);
        const int oi = __shfl_xor(idx, m, FTGP_WAVE);
        if (od < best || (od == best && oi < idx)) { best = od; idx = oi; }
    }
    const int c = idx;
    const int pa = c > 0 ? c - 1 : FTGP_PATH_POINTS - 1;
    FrameSeg g{};
    if (live && l < 2) g = frame_segment(path, l == 0 ? c : pa, x, y);
    const double g2a = shfl_xor_f64(g.g2, 1);                          // lane 0 <- lane 1: segment A's distance
    int take_a = (live && l == 0 && g2a < g.g2) ? 1 : 0;
    take_a = __shfl(take_a, (int)(threadIdx.x & (FTGP_WAVE - 1) & ~(FTGP_FRAME_LANES - 1)), FTGP_WAVE);      // the row's lane 0 tells the row
    if (!live) return;
    const int seg = take_a ? pa : c;
    const double ch = qw * qw - qz * qz, sh = 2.0 * (qw * qz);
    const int width = FTGP_FRAME_FIXED + 2 * F.n_ahead;
    const int k_ext = F.ext_out ? F.ext_index[slot] : -1;
    float* ext = k_ext >= 0 ? F.ext_out + ((size_t)env * F.n_ext + k_ext) * width : nullptr;
    float* row = F.rows ? F.rows + (size_t)ci * width : nullptr;
    if (l == 0) {
        if (take_a) g = frame_segment(path, pa, x, y);
        double s;
        const FrameFixed f = frame_fixed(g, seg, ch, sh, s);
        if (row) { row[0] = f.x; row[1] = f.y; row[2] = f.z; row[3] = f.w; }
        if (ext) { ext[0] = f.x; ext[1] = f.y; ext[2] = f.z; ext[3] = f.w; }
        if (F.s_out) F.s_out[ci] = s;
        if (F.flag_out) F.flag_out[ci] = (best > 1.0 ? FTGP_FRAME_OFF : 0) | (fin ? FTGP_FRAME_FINISHED : 0);
        if (F.c_out) F.c_out[ci] = c;
    }
    if (l < F.n_ahead) {
        const FramePoint p = frame_ahead(path, seg, l, F.stride, x, y, ch, sh);
        if (row) { row[FTGP_FRAME_FIXED + 2 * l] = p.x; row[FTGP_FRAME_FIXED + 2 * l + 1] = p.y; }
        if (ext) { ext[FTGP_FRAME_FIXED + 2 * l] = p.x; ext[FTGP_FRAME_FIXED + 2 * l + 1] = p.y; }
    }
}

// ---------------------------------------------------------------------------------------------
// Rivals (ftgp_device_io_rivals / ftgp_step_device_rivals / ftgp_rivals_device / ftgp_get_rivals): the rival row of include/ftgp.h -- the
// car's place in its env's race, the gaps to the cars around it, and the nearest env-mates in its body frame.  The per-car search
// (s, c, off) is ftgp_io_frame_kernel's, launched just before with s_out, flag_out and c_out.
// ---------------------------------------------------------------------------------------------
struct DeviceRivalArgs {
    const double* s;                      // [n_cars] the unrounded s of every car          } ftgp_io_frame_kernel's outputs
    const int32_t* c;                     // [n_cars] its nearest point                      } at the same records
    const int32_t* flag;                  // [n_cars] FTGP_FRAME_OFF | FTGP_FRAME_FINISHED   }
    float* rows;                          // [n_cars][FTGP_RIVAL_FIXED + 8 * n_rivals]: every car's row, or null
    float* ext_out;                       // [n_envs][n_ext][FTGP_RIVAL_FIXED + 8 * n_rivals]: the external cars' rows, or null
    int32_t* place_out;                   // [n_cars]: the place alone, negated for a finished car (the place reward's p0), or null
    int32_t n_ext, n_rivals;
    int32_t ext_index[FTGP_PAIR_STRIDE];  // as DeviceIoArgs (read with ext_out only)
};

// steps 1 - 4, element by element: ftgp_rival.h (rival_progress, rival_ahead, RivalCar / rival_car, rival_mate)

__device__ __forceinline__ double shfl_f64(double v, int src)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src, FTGP_WAVE);
    hi = __shfl(hi, src, FTGP_WAVE);
    return __hiloint2double(hi, lo);
}

// Eight lanes per car: lane j of a group holds slot j of the car's env (a lane past cars_per_env holds nobody), so a wave holds eight
// cars and a workgroup thirty-two.  Every lane loads its mate's record and the search's results for it and forms g_j and d2_j; place,
// n_racing and the number of mates are sums and the two gaps minima over the group (xor-shuffles 1, 2, 4 stay inside eight lanes);
// a mate's rank is the number of mates before it in (d2, slot) order, counted over the group's eight lanes with plain shuffles.  The
// mate of rank r < n_rivals writes slot r, lane r zero-fills a slot no mate has, lane 0 writes the fixed entries.  No LDS, no atomics.
#define FTGP_RIVAL_THREADS 256
__global__ void __launch_bounds__(FTGP_RIVAL_THREADS) ftgp_io_rival_kernel(DeviceParams P, DeviceRivalArgs V)
{
    // (the car from the block's first car, not from a global lane number: that one would pass 2^31 at 268 M cars)
    const int ci = blockIdx.x * (FTGP_RIVAL_THREADS / FTGP_RIVAL_LANES) + threadIdx.x / FTGP_RIVAL_LANES, j = threadIdx.x % FTGP_RIVAL_LANES;
    const bool live = ci < P.n_cars;
    const int cpe = P.cars_per_env;
    const int env = live ? ci / cpe : 0, slot = live ? ci - env * cpe : 0;
    const bool has = live && j < cpe;            // this lane holds a car of the env
    const bool other = has && j != slot;
    // a lane that holds nobody takes part in the shuffles with these: not ahead, not racing, no mate, no gap
    RivalCar a{}, b{};
    bool fin_a = false, fin_b = false;
    int64_t fs_a = 0, fs_b = 0;
    double g_a = 0.0, g_b = 0.0;
    if (live) {
        const CarCore& r = P.cars[ci];
        const int fl = V.flag[ci];
        a = rival_car(r, V.s[ci]);
        fin_a = r.finished != 0; fs_a = r.finish_step;
        g_a = rival_progress(absolute_completion(r), a.s, V.c[ci], (fl & FTGP_FRAME_OFF) != 0);
    }
    if (has) {
        const int cb = ci - slot + j;
        const CarCore& r = P.cars[cb];
        const int fl = V.flag[cb];
        b = rival_car(r, V.s[cb]);
        fin_b = r.finished != 0; fs_b = r.finish_step;
        g_b = rival_progress(absolute_completion(r), b.s, V.c[cb], (fl & FTGP_FRAME_OFF) != 0);
    }
    const bool ahead = other && rival_ahead(fin_b, fs_b, g_b, j, fin_a, fs_a, g_a, slot);
    const bool mate = other && !fin_b && !fin_a;
    const double dx = b.x - a.x, dy = b.y - a.y;
    const double d2 = dx * dx + dy * dy;
    double gap_ahead = (mate && ahead) ? g_b - g_a : INFINITY;
    double gap_behind = (mate && !ahead) ? g_a - g_b : INFINITY;
    int n_ahead = ahead ? 1 : 0, n_racing = (has && !fin_b) ? 1 : 0, n_mates = mate ? 1 : 0;
    // every lane of the wave is here
    for (int m = 1; m < FTGP_RIVAL_LANES; m <<= 1) {
        const double oa = shfl_xor_f64(gap_ahead, m), ob = shfl_xor_f64(gap_behind, m);
        if (oa < gap_ahead) gap_ahead = oa;
        if (ob < gap_behind) gap_behind = ob;
        n_ahead += __shfl_xor(n_ahead, m, FTGP_WAVE);
        n_racing += __shfl_xor(n_racing, m, FTGP_WAVE);
        n_mates += __shfl_xor(n_mates, m, FTGP_WAVE);
    }
    const int first = (int)(threadIdx.x & (FTGP_WAVE - 1) & ~(FTGP_RIVAL_LANES - 1));      // the group's lane 0 in the wave
    int rank = 0;
    #pragma unroll
    for (int i = 0; i < FTGP_RIVAL_LANES; ++i) {
        const double od = shfl_f64(d2, first + i);
        const int om = __shfl(mate ? 1 : 0, first + i, FTGP_WAVE);
        if (om && (od < d2 || (od == d2 && i < j))) ++rank;
    }
    if (!live) return;
    const int place = 1 + n_ahead;
    if (V.place_out && j == 0) V.place_out[ci] = fin_a ? -place : place;
    const int width = FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * V.n_rivals;
    const int k_ext = V.ext_out ? V.ext_index[slot] : -1;
    float* ext = k_ext >= 0 ? V.ext_out + ((size_t)env * V.n_ext + k_ext) * width : nullptr;
    float* row = V.rows ? V.rows + (size_t)ci * width : nullptr;
    if (j == 0) {
        const float f0 = (float)place, f1 = (float)n_racing, f2 = gap_ahead == INFINITY ? 0.0f : (float)gap_ahead, f3 = gap_behind == INFINITY ? 0.0f : (float)gap_behind;
        if (row) { row[0] = f0; row[1] = f1; row[2] = f2; row[3] = f3; }
        if (ext) { ext[0] = f0; ext[1] = f1; ext[2] = f2; ext[3] = f3; }
    }
    if (mate && rank < V.n_rivals) {
        float o[FTGP_RIVAL_FLOATS];
        rival_mate(a, b, o);
        const int at = FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * rank;
        #pragma unroll
        for (int q = 0; q < FTGP_RIVAL_FLOATS; ++q) {
            if (row) row[at + q] = o[q];
            if (ext) ext[at + q] = o[q];
        }
    }
    if (j >= n_mates && j < V.n_rivals) {        // a slot no mate has
        const int at = FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * j;
        #pragma unroll
        for (int q = 0; q < FTGP_RIVAL_FLOATS; ++q) {
            if (row) row[at + q] = 0.0f;
            if (ext) ext[at + q] = 0.0f;
        }
    }
}

// The rival row by one lane (ftgp_io_finish_signals_kernel, the spawn state of an env it has just reset): what every car of the env
// put into shared memory -- its RivalCar, g, finished and finish_step -- goes through the operations of ftgp_io_rival_kernel.
struct RivalLds { RivalCar car[FTGP_PAIR_STRIDE]; double g[FTGP_PAIR_STRIDE]; int64_t finish_step[FTGP_PAIR_STRIDE]; int32_t finished[FTGP_PAIR_STRIDE]; };

// this lane's car into shared memory: the search as the progress block runs it, steps 2 and 3 of the frame row, step 1 of the rival row
__device__ __forceinline__ void rival_lds_put(const double* __restrict__ path, const CarCore& r, RivalLds& L, int slot)
{
    double s, g;
    rival_place(path, r.x, r.y, absolute_completion(r), s, g);
    L.car[slot] = rival_car(r, s);
    L.g[slot] = g;
    L.finish_step[slot] = r.finish_step;
    L.finished[slot] = r.finished;
}

__device__ __forceinline__ void rival_row_lane(const RivalLds& L, int cpe, int slot, int n_rivals, float* __restrict__ o)
{
    rival_row(L.car, L.g, L.finish_step, L.finished, cpe, slot, n_rivals, o);
}

// ftgp_io_finish_kernel with signals: one workgroup per env.  The rows of obs / final_obs are pooled (pooled_row); an external car that
// is off_track pays the penalty and, with terminate_off_track, ends its env; state rows are written from the records after the steps
// (to final_state for an env that is reset here) and again after the reset.  With contacts on (S.contact_rows, this call's rows of
// ftgp_io_contact_kernel) the wall and car penalties and episode ends join, and the rows go out like the state rows -- zeros after a reset.
// With the frame on (S.frame_rows, this call's rows of ftgp_io_frame_kernel) those rows go out the same way, evaluated again at the spawn
// pose after a reset (frame_row_lane), and with S.frame_s0 the base reward is the dense one.
// With rivals on (S.rival_rows, this call's rows of ftgp_io_rival_kernel) those rows go out like the frame rows, evaluated again at the
// spawn state after a reset (rival_lds_put, rival_row_lane), and with S.place0 the place term joins the reward behind the penalties.
__global__ void __launch_bounds__(FTGP_IO_THREADS) __attribute__((amdgpu_num_vgpr(72))) ftgp_io_finish_signals_kernel(DeviceParams P, DeviceIoArgs A, DeviceSignalArgs S, const FtgpSpawnDev* __restrict__ rule)
{
    __shared__ int ended;
    __shared__ __attribute__((aligned(16))) float stage[FTGP_SIG_STAGE_FLOATS];
    __shared__ RivalLds rival_lds;
    const int env = blockIdx.x, cpe = P.cars_per_env, ci0 = env * cpe, t = threadIdx.x;
    if (t == 0) {
        bool all_finished = true, off = false, wall = false, car = false;
        for (int c = 0; c < cpe; ++c)
            if (A.ext_index[c] >= 0) {
                if (!P.cars[ci0 + c].finished) all_finished = false;
                if (P.cars[ci0 + c].off_track) off = true;
                if (S.contact_rows) {
                    const float* cr = S.contact_rows + (size_t)(ci0 + c) * FTGP_CONTACT_FLOATS;
                    if (cr[2] > 0.0f) wall = true;
                    if (cr[3] > 0.0f) car = true;
                }
            }
        const bool term = all_finished || (S.terminate_off_track && off) || (S.terminate_on_wall && wall) || (S.terminate_on_car && car);
        const bool trunc = !term && A.max_episode_steps > 0 && P.steps[env] >= A.max_episode_steps;
        A.terminated[env] = term ? 1 : 0;
        A.truncated[env] = trunc ? 1 : 0;
        ended = (term || trunc) ? 1 : 0;
    }
    const bool mine = t < cpe && A.ext_index[t] >= 0;
    const size_t my_row = (size_t)env * A.n_ext + (mine ? A.ext_index[t] : 0);
    if (mine) {
        const CarCore& a = P.cars[ci0 + t];
        float r = (float)(absolute_completion(a) - A.prev_abs[ci0 + t]);
        if (S.frame_s0) {          // dense progress: the change of s over the call, frozen off the track and for a car that had finished
            const int f0 = S.frame_flag0[ci0 + t], f1 = S.frame_flag1[ci0 + t];
            double ds = S.frame_s1[ci0 + t] - S.frame_s0[ci0 + t];
            if (ds >= 50.0) ds = ds - 100.0;
            if (ds < -50.0) ds = ds + 100.0;
            if ((f0 & (FTGP_FRAME_OFF | FTGP_FRAME_FINISHED)) || (f1 & FTGP_FRAME_OFF)) ds = 0.0;
            r = (float)ds;
        }
        if (a.off_track) r = r - S.penalty;
        if (S.contact_rows) {
            const float* cr = S.contact_rows + (size_t)(ci0 + t) * FTGP_CONTACT_FLOATS;
            if (cr[2] > 0.0f) r = r - S.wall_penalty;
            if (cr[3] > 0.0f) r = r - S.car_penalty;
        }
        if (S.place0) {            // place reward: places gained over the call, nothing for a car that had finished
            const int p0 = S.place0[ci0 + t], p1 = (int)S.rival_rows[(size_t)(ci0 + t) * (FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * S.rival_n)];
            const float gained = (float)(p0 < 0 ? 0 : p0 - p1);
            const float term = S.place_weight * gained;
            r = r + term;
        }
        A.reward[my_row] = r;
    }
    __syncthreads();
    const bool reset = A.auto_reset && ended;
    if (mine) {
        float* dst = reset ? S.final_state : S.state;
        if (dst) state_row(P.cars[ci0 + t], dst + my_row * FTGP_STATE_FLOATS);
        if (S.contact_rows) {
            const float* cr = S.contact_rows + (size_t)(ci0 + t) * FTGP_CONTACT_FLOATS;
            float* row = reset ? S.final_contact : S.contact;
            if (row) for (int q = 0; q < FTGP_CONTACT_FLOATS; ++q) row[my_row * FTGP_CONTACT_FLOATS + q] = cr[q];
            if (reset && S.contact) for (int q = 0; q < FTGP_CONTACT_FLOATS; ++q) S.contact[my_row * FTGP_CONTACT_FLOATS + q] = 0.0f;
        }
        if (S.frame_rows) {
            const int width = FTGP_FRAME_FIXED + 2 * S.frame_ahead;
            const float* fr = S.frame_rows + (size_t)(ci0 + t) * width;
            float* row = reset ? S.final_frame : S.frame;
            if (row) for (int q = 0; q < width; ++q) row[my_row * width + q] = fr[q];
        }
        if (S.rival_rows) {
            const int width = FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * S.rival_n;
            const float* rr = S.rival_rows + (size_t)(ci0 + t) * width;
            float* row = reset ? S.final_rival : S.rival;
            if (row) for (int q = 0; q < width; ++q) row[my_row * width + q] = rr[q];
        }
    }
    const int R = P.n_rays, NB = S.n_beams;
    for (int c = 0; c < cpe; ++c) {
        const int k = A.ext_index[c];
        float* src = P.ranges + (size_t)(ci0 + c) * P.ranges_stride;
        if (k >= 0) {
            const size_t row = ((size_t)env * A.n_ext + k) * NB;
            float* obs = A.obs + row;
            float* dst = !reset ? obs : A.final_obs ? A.final_obs + row : nullptr;      // one call site: the row's code exists once
            if (dst) pooled_row(src, dst, R, S, stage);
            if (reset) {
                if (S.vec_out) for (int j = t; j < NB / 4; j += FTGP_IO_THREADS) reinterpret_cast<float4*>(obs)[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                else for (int j = t; j < NB; j += FTGP_IO_THREADS) obs[j] = 0.0f;
            }
        }
        __syncthreads();      // the row has been read before it is zeroed
        if (reset) for (int j = t; j < P.ranges_stride; j += FTGP_IO_THREADS) src[j] = 0.0f;
    }
    // spawn rule: every lane reads the env's episode counter, and a barrier separates the reads from lane 0 advancing it
    int64_t episode = 0;
    if (reset && rule) {          // (both uniform over the workgroup)
        episode = rule->episodes[env];
        __syncthreads();
    }
    if (reset && t < cpe) {
        reset_car(P, ci0 + t, A.env_track, rule, episode);      // (the records were read before the first barrier, and by this lane above)
        if (mine && S.state) state_row(P.cars[ci0 + t], S.state + my_row * FTGP_STATE_FLOATS);
        if (mine && S.frame_rows && S.frame)      // the frame at the spawn pose: a look-ahead of zeros would be a lie
            frame_row_lane(P.path + (size_t)env_track_of(A.env_track, env) * 2 * FTGP_PATH_POINTS, P.cars[ci0 + t], S.frame_ahead, S.frame_stride,
                           S.frame + my_row * (FTGP_FRAME_FIXED + 2 * S.frame_ahead));
        if (t == 0 && rule) rule->episodes[env] = episode + 1;
    }
    if (reset && S.rival_rows && S.rival) {      // (uniform over the workgroup) the rival rows at the spawn state: every car's inputs, then the external cars' rows
        if (t < cpe) rival_lds_put(P.path + (size_t)env_track_of(A.env_track, env) * 2 * FTGP_PATH_POINTS, P.cars[ci0 + t], rival_lds, t);
        __syncthreads();
        if (mine) rival_row_lane(rival_lds, cpe, t, S.rival_n, S.rival + my_row * (FTGP_RIVAL_FIXED + FTGP_RIVAL_FLOATS * S.rival_n));
    }
}

// ftgp_obs_device: the external cars' observation rows at the scans as they stand, one workgroup per env -- pooled_row as the finish
// kernel above calls it, so a row is what a step's obs holds for those scans.  (ftgp_io_finish_kernel copies the scans as they are;
// pool 1 without a clip gives the same bits for every range a sweep writes: a hit >= 0, or -1.)
__global__ void __launch_bounds__(FTGP_IO_THREADS) ftgp_io_obs_kernel(DeviceParams P, DeviceIoArgs A, DeviceSignalArgs S)
{
    __shared__ __attribute__((aligned(16))) float stage[FTGP_SIG_STAGE_FLOATS];
    const int env = blockIdx.x, cpe = P.cars_per_env, ci0 = env * cpe;
    for (int c = 0; c < cpe; ++c) {
        const int k = A.ext_index[c];
        if (k < 0) continue;      // (uniform over the workgroup)
        pooled_row(P.ranges + (size_t)(ci0 + c) * P.ranges_stride, A.obs + ((size_t)env * A.n_ext + k) * S.n_beams, P.n_rays, S, stage);
    }
}

// ---------------------------------------------------------------------------------------------
// Env states (ftgp_save_envs_device / ftgp_load_envs_device): the record of include/ftgp.h -- header, steps and episodes, the car
// records, the dynamics records, the scans -- gathered from / scattered to the handle's five state arrays.  A wave per env, the env
// index wave-uniform; every part starts on a 16-byte boundary on both sides, so a part moves as uint4, lane i taking vector i, i + 64,
// ...: a wave's loads and stores cover consecutive 1 KiB.  No LDS, no scratch, nothing indexed by a lane but global memory.
// ---------------------------------------------------------------------------------------------
#define FTGP_ENV_STATE_THREADS 256
#define FTGP_ENV_STATE_HEAD 3                             // uint4: magic version n_rays cars | lidar_mode 0 fingerprint | steps episodes
#define FTGP_CAR_VEC ((int)(sizeof(CarState) / 16))
#define FTGP_DYN_VEC ((int)(FTGP_DYN_RECORD * sizeof(double) / 16))
static_assert(sizeof(CarState) % 16 == 0 && (FTGP_DYN_RECORD * sizeof(double)) % 16 == 0, "the parts of an env-state record move as uint4");
static_assert(sizeof(CarState) == 448 && offsetof(CarCore, completion) == 136 && offsetof(CarCore, start) == 168 && sizeof(CarCore) == 192,
              "the car record of an env-state record is part of the interface (include/ftgp.h)");

// what a handle's first save or load puts into device memory
struct EnvStateAux {
    double own[FTGP_DYN_RECORD];              // the handle's own dynamics record: what a save writes while the table is off
    unsigned long long rejected, pad;         // rows a load has refused
    uint64_t track_fp[FTGP_MAX_TRACKS];       // the tracks' fingerprints
};
static_assert(offsetof(EnvStateAux, own) == 0 && offsetof(EnvStateAux, rejected) % 16 == 0, "EnvStateAux layout");

struct EnvStateArgs {
    uint4* rows;                  // [n_rows][env_vec] the caller's records (a load only reads them)
    int64_t n_rows;
    const uint8_t* env_mask;      // save: [n_envs] or null = all envs
    const int32_t* src_row;       // load: [n_envs] or null = row e
    const int32_t* env_track;     // the track of every env; null with one track
    EnvStateAux* aux;
    int64_t* episodes;            // [n_envs]; null on a handle that never had a spawn rule
    uint4* dyn;                   // the dynamics records; null while the table is off
    int32_t row_vec;              // uint4 per scan row of a record: pad16(4 n_rays) / 16
    int32_t env_vec;              // uint4 per record
};

__device__ __forceinline__ int env_state_env() { return sgpr((int)(blockIdx.x * (FTGP_ENV_STATE_THREADS / FTGP_WAVE) + threadIdx.x / FTGP_WAVE)); }

__global__ void __launch_bounds__(FTGP_ENV_STATE_THREADS) ftgp_env_save_kernel(DeviceParams P, EnvStateArgs A)
{
    const int env = env_state_env();
    if (env >= P.n_envs) return;
    if (A.env_mask && !A.env_mask[env]) return;
    const int lane = lane_id(), cpe = P.cars_per_env;
    uint4* o = A.rows + (size_t)env * (size_t)A.env_vec;
    if (lane < FTGP_ENV_STATE_HEAD) {
        const uint64_t fp = A.aux->track_fp[env_track_of(A.env_track, env)];
        const uint64_t steps = (uint64_t)P.steps[env], episodes = A.episodes ? (uint64_t)A.episodes[env] : 0ull;
        uint4 v = make_uint4(FTGP_ENV_STATE_MAGIC, FTGP_ENV_STATE_VERSION, (uint32_t)P.n_rays, (uint32_t)cpe);
        if (lane == 1) v = make_uint4((uint32_t)P.lidar_mode, 0u, (uint32_t)fp, (uint32_t)(fp >> 32));
        if (lane == 2) v = make_uint4((uint32_t)steps, (uint32_t)(steps >> 32), (uint32_t)episodes, (uint32_t)(episodes >> 32));
        o[lane] = v;
    }
    o += FTGP_ENV_STATE_HEAD;
    const int n_car = cpe * FTGP_CAR_VEC, n_dyn = cpe * FTGP_DYN_VEC;
    const uint4* cars = reinterpret_cast<const uint4*>(P.cars + (size_t)env * cpe);
    for (int i = lane; i < n_car; i += FTGP_WAVE) o[i] = cars[i];
    o += n_car;
    if (A.dyn) {
        const uint4* dyn = A.dyn + (size_t)env * n_dyn;
        for (int i = lane; i < n_dyn; i += FTGP_WAVE) o[i] = dyn[i];
    } else {
        const uint4* own = reinterpret_cast<const uint4*>(A.aux->own);
        for (int i = lane; i < n_dyn; i += FTGP_WAVE) o[i] = own[i % FTGP_DYN_VEC];
    }
    o += n_dyn;
    for (int c = 0; c < cpe; ++c) {
        // (a scan row in the handle is ranges_stride floats, a multiple of 32 >= n_rays: the last vector of a record's row lies inside it)
        const uint4* src = reinterpret_cast<const uint4*>(P.ranges + (size_t)(env * cpe + c) * P.ranges_stride);
        for (int j = lane; j < A.row_vec; j += FTGP_WAVE) {
            uint4 v = src[j];
            const int left = P.n_rays - 4 * j;        // rays from this vector on, >= 1: zeros behind the row's last ray
            if (left < 4) v.w = 0u;
            if (left < 3) v.z = 0u;
            if (left < 2) v.y = 0u;
            o[(size_t)c * A.row_vec + j] = v;
        }
    }
}

// The header is compared before the first store: an env is loaded whole or not at all.
__global__ void __launch_bounds__(FTGP_ENV_STATE_THREADS) ftgp_env_load_kernel(DeviceParams P, EnvStateArgs A)
{
    const int env = env_state_env();
    if (env >= P.n_envs) return;
    const int r = A.src_row ? sgpr(A.src_row[env]) : env;
    if (r < 0) return;
    const int lane = lane_id(), cpe = P.cars_per_env;
    bool ok = (int64_t)r < A.n_rows;
    const uint4* s = A.rows + (ok ? (size_t)r * (size_t)A.env_vec : 0);
    uint4 h2 = make_uint4(0u, 0u, 0u, 0u);
    if (ok) {
        const uint4 h0 = s[0], h1 = s[1];
        h2 = s[2];
        const uint64_t fp = A.aux->track_fp[env_track_of(A.env_track, env)];
        ok = h0.x == FTGP_ENV_STATE_MAGIC && h0.y == FTGP_ENV_STATE_VERSION && h0.z == (uint32_t)P.n_rays && h0.w == (uint32_t)cpe &&
             h1.x == (uint32_t)P.lidar_mode && h1.z == (uint32_t)fp && h1.w == (uint32_t)(fp >> 32);
    }
    if (!ok) {
        if (lane == 0) atomicAdd(&A.aux->rejected, 1ull);
        return;
    }
    if (lane == 0) {
        P.steps[env] = (int64_t)(((uint64_t)h2.y << 32) | h2.x);
        if (A.episodes) A.episodes[env] = (int64_t)(((uint64_t)h2.w << 32) | h2.z);
    }
    s += FTGP_ENV_STATE_HEAD;
    const int n_car = cpe * FTGP_CAR_VEC, n_dyn = cpe * FTGP_DYN_VEC;
    uint4* cars = reinterpret_cast<uint4*>(P.cars + (size_t)env * cpe);
    for (int i = lane; i < n_car; i += FTGP_WAVE) cars[i] = s[i];
    s += n_car;
    if (A.dyn) {
        uint4* dyn = A.dyn + (size_t)env * n_dyn;
        for (int i = lane; i < n_dyn; i += FTGP_WAVE) dyn[i] = s[i];
    }
    s += n_dyn;
    const int whole = P.n_rays / 4, tail = P.n_rays % 4;
    for (int c = 0; c < cpe; ++c) {
        float* dst = P.ranges + (size_t)(env * cpe + c) * P.ranges_stride;
        const uint4* row = s + (size_t)c * A.row_vec;
        for (int j = lane; j < whole; j += FTGP_WAVE) reinterpret_cast<uint4*>(dst)[j] = row[j];
        if (tail && lane == whole % FTGP_WAVE) {          // the row's last one to three rays: what lies behind them in the handle stays
            const uint4 v = row[whole];
            dst[4 * whole] = __uint_as_float(v.x);
            if (tail > 1) dst[4 * whole + 1] = __uint_as_float(v.y);
            if (tail > 2) dst[4 * whole + 2] = __uint_as_float(v.z);
        }
    }
}

// Packed read-back rows, one car per lane: the host copies 3 small arrays instead of the whole state records.
//   prog  int32[n_cars][FTGP_PROGRESS_INTS]   (custom.py:91-143: lap_completion / absolute_completion folded in)
//   core  double[n_cars][16]: x y qw qz vx vy wz u_speed u_steer laps lap_completion absolute_completion steps n_times start finish_step (the last two: int64 bit patterns)
__global__ void ftgp_pack_kernel(DeviceParams P, int32_t* __restrict__ prog, double* __restrict__ core)
{
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= P.n_cars) return;
    const CarState& a = P.cars[ci];
    const int lc = a.good_start ? a.completion : -(100 - a.completion);         // custom.py:132-140
    int32_t* o = prog + (size_t)ci * FTGP_PROGRESS_INTS;
    o[0] = a.laps; o[1] = a.completion; o[2] = lc; o[3] = a.laps * 100 + lc; o[4] = a.finished;   // custom.py:142-143
    // the row is int32 while steps are int64: start and finish_step saturate at 2^31 - 1 here (ftgp_get_race_steps has all 64 bits)
    const int64_t top = 0x7fffffffll;
    o[5] = a.off_track; o[6] = (int32_t)(a.start > top ? top : a.start); o[7] = a.good_start; o[8] = a.delta;
    o[9] = a.finished ? (int32_t)(a.finish_step > top ? top : a.finish_step) : -1;
    double* d = core + (size_t)ci * 16;
    d[0] = a.x; d[1] = a.y; d[2] = a.qw; d[3] = a.qz; d[4] = a.vx; d[5] = a.vy; d[6] = a.wz; d[7] = a.u_speed; d[8] = a.u_steer;
    d[9] = a.laps; d[10] = lc; d[11] = a.laps * 100 + lc; d[12] = (double)P.steps[ci / P.cars_per_env]; d[13] = a.n_times;
    d[14] = __longlong_as_double(a.start); d[15] = __longlong_as_double(a.finished ? a.finish_step : -1ll);      // bit patterns of the two int64 (ftgp_get_race_steps)
}

// fakelidar-compat (raycast.py:5-21): one ray per lane, binary64, same operation order as the Python loop.
__global__ void ftgp_fakelidar_kernel(const double* __restrict__ dt, int H, int W, int n_rays_total, int R,
                                      const double* __restrict__ origins, const double* __restrict__ cosines, const double* __restrict__ sines,
                                      double eps, double* __restrict__ scan, double* __restrict__ points, int* __restrict__ index_error)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays_total) return;
    const int o = i / R;
    double x = origins[2 * o], y = origins[2 * o + 1];
    const double dx = cosines[i], dy = sines[i];
    double distance = 0.0;
    bool bad = false;
    long yi = (long)y, xi = (long)x;                          // int(): truncation toward zero
    if (yi < 0) yi += H;
    if (xi < 0) xi += W;                                      // numpy negative-index wrap
    double nearest = 0.0;
    if (yi < 0 || yi >= H || xi < 0 || xi >= W) bad = true; else nearest = dt[(size_t)yi * W + xi];
    for (int guard = 0; guard < (1 << 20) && !bad && nearest > eps && 0 <= x && x <= W && 0 <= y && y <= H; ++guard) {
        distance += nearest;
        x += dx * nearest;
        y += dy * nearest;
        yi = (long)y; xi = (long)x;
        if (yi < 0) yi += H;
        if (xi < 0) xi += W;
        if (yi < 0 || yi >= H || xi < 0 || xi >= W) { bad = true; break; }
        nearest = dt[(size_t)yi * W + xi];
    }
    if (bad) atomicOr(index_error, 1);
    scan[i] = distance; points[2 * i] = x; points[2 * i + 1] = y;
}

// Sector box field build (ftgp_create): one cell of one plane per lane, ring included.
__global__ void ftgp_box_field_kernel(const uint16_t* __restrict__ runx, const uint16_t* __restrict__ runy, int W, int H, int n_sectors, uint16_t* __restrict__ out)
{
    const size_t cells = (size_t)ftgp_plane256(W, H) * 128;          // 16-bit entries per (padded) plane
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells * (size_t)n_sectors) return;
    const int sector = (int)(i / cells);
    const size_t c = i - (size_t)sector * cells;
    const int X = (int)(c % (size_t)(W + 2)), Y = (int)(c / (size_t)(W + 2));
    uint32_t e = FTGP_FIELD_OUT;
    if (X >= 1 && X <= W && Y >= 1 && Y <= H) e = ftgp_box_entry(runx, runy, W, H, X - 1, Y - 1, sector, n_sectors / 8);
    out[i] = (uint16_t)e;
}

// Exact Euclidean distance transform (FTGP_LIDAR_FAKELIDAR): out[y][x] = distance from pixel (x, y) to the nearest wall pixel,
// centre to centre, 0 on walls -- scipy.ndimage.distance_transform_edt(~wall), the recipe of custom.py:1149-1153 / raycast.py:24-27.
// runy[d][y][x] = wall-free run from the pixel along +y (d = 0) / -y (d = 1), 0 on walls, 65535 = to the image edge, so
// g(x', y) = min of the two is the vertical distance to the nearest wall of column x'.  One pixel per lane walks its row outwards
// from x until (x - x')^2 alone reaches the best squared distance: integers throughout, then one correctly rounded sqrt.
__global__ void ftgp_edt_kernel(const uint16_t* __restrict__ runy, int W, int H, double* __restrict__ out)
{
    const size_t plane = (size_t)W * H;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int x = (int)(i % (size_t)W);
    const uint16_t* up = runy + (i - x), * down = runy + plane + (i - x);       // the pixel's row in both planes
    const long long INF = 1ll << 40;
    long long best = INF;
    for (int k = 0; k < W; ++k) {
        const long long k2 = (long long)k * k;
        if (k2 >= best) break;
        for (int sgn = 0; sgn < (k ? 2 : 1); ++sgn) {
            const int xp = sgn ? x + k : x - k;
            if (xp < 0 || xp >= W) continue;
            const int g = min((int)up[xp], (int)down[xp]);
            if (g == 65535) continue;                                            // no wall in that column
            const long long d2 = k2 + (long long)g * g;
            best = d2 < best ? d2 : best;
        }
    }
    out[i] = sqrt((double)best);
}

// Metrics record (FTGP_METRIC_DOUBLES): one block of 1024 threads (a handful of cars each: the records are 448 B apart, so the
// loads want to be in flight together); reduction inside each wave by shuffles, then across the 16 waves through LDS.  The
// sums are integers, exact in binary64 in any order.
#define FTGP_METRIC_THREADS 1024
__global__ void __launch_bounds__(FTGP_METRIC_THREADS) ftgp_metrics_kernel(DeviceParams P, double* __restrict__ out)
{
    __shared__ double part[7][FTGP_METRIC_THREADS / FTGP_WAVE];
    double steps = 0, laps = 0, absc = 0, fin = 0, off = 0, tmin = INFINITY, tmax = -INFINITY;
    for (int e = threadIdx.x; e < P.n_envs; e += blockDim.x) steps += (double)P.steps[e];
    for (int i = threadIdx.x; i < P.n_cars; i += blockDim.x) {
        const CarState& a = P.cars[i];
        const int lc = a.good_start ? a.completion : -(100 - a.completion);     // custom.py:132-143
        laps += a.laps; absc += a.laps * 100 + lc; fin += a.finished; off += a.off_track;
        const int n = a.n_times < FTGP_MAX_LAP_TIMES ? a.n_times : FTGP_MAX_LAP_TIMES;
        for (int k = 0; k < n; ++k) { tmin = fmin(tmin, a.times[k]); tmax = fmax(tmax, a.times[k]); }
    }
    const int lane = threadIdx.x & (FTGP_WAVE - 1), wave = threadIdx.x >> 6;
    steps = wave_sum_f64(steps); laps = wave_sum_f64(laps); absc = wave_sum_f64(absc); fin = wave_sum_f64(fin); off = wave_sum_f64(off);
    #pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { tmin = fmin(tmin, shfl_xor_f64(tmin, m)); tmax = fmax(tmax, shfl_xor_f64(tmax, m)); }
    if (lane == 0) { part[0][wave] = steps; part[1][wave] = laps; part[2][wave] = absc; part[3][wave] = fin; part[4][wave] = off; part[5][wave] = tmin; part[6][wave] = tmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[7] = { 0, 0, 0, 0, 0, INFINITY, -INFINITY };
        for (int w = 0; w < FTGP_METRIC_THREADS / FTGP_WAVE; ++w) {
            for (int q = 0; q < 5; ++q) r[q] += part[q][w];
            r[5] = fmin(r[5], part[5][w]); r[6] = fmax(r[6], part[6][w]);
        }
        out[0] = r[0]; out[1] = (double)P.n_cars; out[2] = r[1]; out[3] = r[2];
        out[4] = r[3]; out[5] = r[4]; out[6] = r[5]; out[7] = r[6];
    }
}

// =============================================================================================
// Collected rollouts with values (include/ftgp.h: ftgp_collect_values_device, ftgp_gae_device).  Behind every other kernel of the file, so
// that the code object keeps the others where they were.
// =============================================================================================
template __global__ void ftgp_collect_act_kernel<true, true>(DeviceParams, CollectValueArgs);
template __global__ void ftgp_collect_act_kernel<false, true>(DeviceParams, CollectValueArgs);

// The advantage scan: one thread per row (env, external car), t descending, so that a wave's loads of one t are contiguous; the element
// step is ftgp_gae_step of ftgp_net.h, which tools/collect_values_check.cpp compiles for the CPU.
struct GaeArgs {
    const float* reward; const float* value; const float* next_value;      // [T][n_rows]
    const uint8_t* terminated; const uint8_t* truncated;                   // [T][n_envs]
    float* advantage; float* ret;                                          // [T][n_rows]
    float gamma, gl;              // gl = gamma * lam, rounded once on the host
    int32_t T, n_rows, n_ext, n_envs;
};
__global__ void __launch_bounds__(256) ftgp_gae_kernel(GaeArgs G)
{
    const int row = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (row >= G.n_rows) return;
    const int env = row / G.n_ext;
    float a = 0.0f;
    for (int t = G.T - 1; t >= 0; --t) {
        const size_t at = (size_t)t * (size_t)G.n_rows + (size_t)row, ae = (size_t)t * (size_t)G.n_envs + (size_t)env;
        const float v = G.value[at];
        a = ftgp_gae_step(G.gamma, G.gl, G.reward[at], v, G.next_value[at], G.terminated[ae] != 0, G.truncated[ae] != 0, t == G.T - 1, a);
        G.advantage[at] = a;
        G.ret[at] = ftgp_gae_return(a, v);
    }
}

// =============================================================================================
// Training on the device (include/ftgp.h: ftgp_train_grad_device, ftgp_train_adam_device).  Behind every other kernel of the file, so that
// the code object keeps the others where they were.
// =============================================================================================
#include "ftgp_train.h"
