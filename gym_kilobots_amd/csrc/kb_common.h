// kb_common.h -- constants, kernel parameters and device helpers shared by the translation units (the LDS layout: kb_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "kilobots_hip.h"
#include "kb_launch.h"
#include "kb_exact.h"

namespace kb {

// ---- Box2D 2.3.1 constants (b2Settings.h) ---------------------------------------------------
constexpr float B2_PI = 3.14159265359f;
constexpr float B2_LINEAR_SLOP = 0.005f;
constexpr float B2_POLYGON_RADIUS = 2.0f * B2_LINEAR_SLOP;
constexpr float B2_BAUMGARTE = 0.2f;
constexpr float B2_MAX_LINEAR_CORRECTION = 0.2f;
constexpr float B2_MAX_TRANSLATION = 2.0f;
constexpr float B2_MAX_TRANSLATION_SQ = B2_MAX_TRANSLATION * B2_MAX_TRANSLATION;
constexpr float B2_MAX_ROTATION = 0.5f * B2_PI;
constexpr float B2_MAX_ROTATION_SQ = B2_MAX_ROTATION * B2_MAX_ROTATION;
constexpr float B2_EPSILON = 1.19209290e-07f;
constexpr float B2_TOI_BAUMGARTE = 0.75f;
constexpr int B2_MAX_SUBSTEPS = 8;     // b2World::SolveTOI k_maxSubSteps
constexpr float B2_TIME_TO_SLEEP = 0.5f;                                  // b2_timeToSleep
constexpr float B2_LINEAR_SLEEP_TOL = 0.01f;                              // b2_linearSleepTolerance
constexpr float B2_ANGULAR_SLEEP_TOL = 2.0f / 180.0f * B2_PI;             // b2_angularSleepTolerance
constexpr float WORLD_SCALE = 25.0f;  // body.py:7

constexpr float CELL_SIZE = 0.875f;   // world units, >= 2 * bot radius
constexpr int MAX_CELLS = 8192;

constexpr unsigned KEY_WALL = 0x10000u, KEY_OBJ = 0x20000u;
constexpr int WALL_CODE = 0xFFF0;     // body id of wall w is WALL_CODE + w
constexpr int OBJ_CODE = 0xFFE0;      // 16-bit warm-start key of object m (its body id is N + m)
constexpr int MAXOBJ = KB_MAX_OBJECTS;
constexpr unsigned short EMPTY16 = 0xFFFFu;

#ifndef KB_KREG
#define KB_KREG 2
#endif
constexpr int MAX_BUCKETS = MAX_WAVES * BK_PER_WAVE;
constexpr int GIANT_ISLAND = 256;     // contacts; larger islands are swept by the whole workgroup
constexpr int BIG_ISLAND = 16;        // contacts; islands from this size on are placed on waves one by one when the hash placement overloads a wave
constexpr int KREG = KB_KREG;               // contacts a lane can keep in registers (register-resident solver)
#ifndef KB_NSOLVE_DIV
#define KB_NSOLVE_DIV 1                 // sweeping waves = waves of the workgroup / KB_NSOLVE_DIV (A/B knob, see kb_regsolve_bins.inc)
#endif
#ifndef KB_KREG_BINS
#define KB_KREG_BINS (2 * KB_NSOLVE_DIV)                  // ... in the kernels without objects, where only half the waves of a workgroup sweep (kb_regsolve_bins.inc)
#endif
#ifndef KB_SETUP_FUSED
#define KB_SETUP_FUSED 2                // register set-up of a wave of at most 64 contacts (A/B knob, see kb_regsolve_bins.inc): 0 = as a two-slot wave; 1 = one slot, loaded once; 2 = ... and its warm start rides in the depth rounds
#endif

#ifndef KB_ARGS_SCOPED
#define KB_ARGS_SCOPED 1                // fixed-size kernels without objects: arguments re-read per phase (A/B knob, see kb_step_kernel.h: KB_REARG); 0 = carried from the kernel top
#endif

enum { M_NCON = 0, M_TOTAL = 1, M_ANY = 2, M_STATUS = 3, M_MAXISL = 4, M_PROF = 5, M_XTRA = 6, M_XFILL = 7, M_WCNT = 8, M_WAKE = 32 /* .. 63: one bit per kilobot (sleeping; the -DKB_PROFILE build keeps its stamps there and does not implement the wake rule) */, M_WFILL = 8 + MAX_WAVES, M_COUNT = 8 + 2 * MAX_WAVES };
static_assert(M_COUNT <= 64, "misc area");

struct Params {
    kb_buffers buf;
    const float *actions;
    const float *light_action;
    int N, NP, NB, M, E, S, gw, gh, ncell, cap, capL, n_substeps, flags, drive_mode, light_type, vel_iters, pos_iters;
    int solver_mode, toi_walls;
    float xmin, ymin, xmax, ymax, inv_cell, r_bot, im_bot, kl_bot, ka_bot, h;
    float light_radius, light_lo[2], light_hi[2], act_lo[2], act_hi[2];
    // general light model (GradientLight / MomentumLight / CompositeLight): per component
    int lcount, ladim, lkind[KB_MAX_LIGHTS];
    float lradius[KB_MAX_LIGHTS], lmaxv[KB_MAX_LIGHTS];
    float llo[KB_MAX_LIGHTS][2], lhi[KB_MAX_LIGHTS][2], lalo[KB_MAX_LIGHTS][2], lahi[KB_MAX_LIGHTS][2];
    float kl_obj, ka_obj;
    float otab[KB_MAX_OBJECTS][OT_WORDS_C];   // fixture table (kb_objects.h: OT_*)
    float obody[KB_MAX_OBJECTS][BT_WORDS_C];  // body table (kb_objects.h: BT_*)
    int F;                                    // fixtures (>= M)
    float mu_oo, mu_ow;                       // b2MixFriction: object-object, object-wall
    int nmc;                                  // manifold-constraint candidates: pairs + 4 walls per object
    int lds_total;
    int nhead, hmask;                         // cell heads: nhead entries; hmask != 0: a hash table of the cells (slot = cell & hmask)
    int allow_sleep;                          // kb_config.allow_sleep: the SLEEP instantiations are launched
    float im_mode[5];                         // KB_DRIVE_MIXED: inverse mass of a kilobot by drive law
    int botlaw_off;                           // ... and the LDS offset of the per-kilobot law bytes (behind the image)
    int islmin_off;                           // sorted-bin image, SLEEP: LDS offset of the per-island minimum of the sleep times (NB words)
    int sense_s;                              // IR neighbour sensing: reach of the stencil in cells (0 = off)
    float sense_r2;                           // ... and the squared radius in world units
    // uniform constants of the contact search and the solver, evaluated once on the host (same fp32 expressions): as kernel
    // arguments they live in scalar registers -- computed in the kernel they would hold a vector register each
    float rr2, rw2, rw_tot;                   // (r + r)^2;  (polygonRadius + r)^2;  r + polygonRadius (no kernel reads it: kb_create makes toi_tt of it)
    float toi_tt;                             // target + tolerance of kb_toi_wall for a kilobot, by its operations (kb_toi_no_event)
    float nm_bb, nm_wb;                       // effective mass of a kilobot-kilobot and of a wall-kilobot contact
    float y_bb, y_wb;                         // RN(1 / (im_bot + im_bot)), RN(1 / im_bot): the position sweep divides by multiplying (kb_exact.h) ...
    int exact_div;                            // ... once kb_create has checked kb_div_const against a / K for these two K; 0: the sweep divides
    const unsigned char *env_mask;            // kb_step_envs: [E] bytes, set per launch like `actions`; an env whose byte is 0 is not stepped.  NULL: every env
};


// ---- device math ----------------------------------------------------------------------------
// sin/cos: Cephes single-precision algorithm (argument reduction by pi/4 in three parts, degree-3
// minimax polynomials in x^2).  Own implementation so that results are identical wherever the
// same specification is evaluated in IEEE fp32.
__device__ __forceinline__ void kb_sincosf(float xx, float &sn, float &cs) {
    const float DP1 = 0.78515625f, DP2 = 2.4187564849853515625e-4f, DP3 = 3.77489497744594108e-8f;
    const float FOPI = 1.27323954473516f;
    float x = fabsf(xx);
    int j = (int)(FOPI * x);
    float y = (float)j;
    if (j & 1) { j += 1; y += 1.0f; }
    j &= 7;
    float ssign = xx < 0.0f ? -1.0f : 1.0f, csign = 1.0f;
    if (j > 3) { ssign = -ssign; csign = -csign; j -= 4; }
    if (j > 1) csign = -csign;
    x = ((x - y * DP1) - y * DP2) - y * DP3;
    float z = x * x;
    float pc = ((2.443315711809948E-005f * z - 1.388731625493765E-003f) * z + 4.166664568298827E-002f) * z * z
               - 0.5f * z + 1.0f;
    float ps = ((-1.9515295891E-4f * z + 8.3321608736E-3f) * z - 1.6666654611E-1f) * z * x + x;
    if (j == 1 || j == 2) { sn = ssign * pc; cs = csign * ps; }
    else { sn = ssign * ps; cs = csign * pc; }
}

// CircularGradientLight.value_and_gradients, light.py:176-189 (zero gradient instead of NaN at distance 0)
__device__ __forceinline__ void kb_light_circular(float sx, float sy, float lx, float ly, float R,
                                                  float &val, float &gx, float &gy) {
    float dx = -1.0f * (sx - lx), dy = -1.0f * (sy - ly);
    float n = sqrtf(dx * dx + dy * dy);
    float v = 1.0f - n / R;
    v = fmaxf(fminf(v, 1.0f), 0.0f);
    val = v * 255.0f;
    if (n > 0.0f) { dx = dx / n; dy = dy / n; }
    else { dx = 0.0f; dy = 0.0f; }
    if (n > R) { dx *= 0.0f; dy *= 0.0f; }
    gx = dx; gy = dy;
}

// ---- light models shared by the step kernel and kb_light_sense (same operations in the same order: same bits) ----
// (AR: Params, or Params in the constant address space -- the kernel-argument segment itself, kb_step_kernel.h: KB_REARG)
// SinglePositionLight.step of the single circular light, light.py:59-75; la = this env's action (2 floats)
template <class AR>
__device__ __forceinline__ void kb_light_single_step(const AR &p, const float *la, float h, float &lx, float &ly) {
    float ax = fminf(fmaxf(la[0], p.act_lo[0]), p.act_hi[0]);
    float ay = fminf(fmaxf(la[1], p.act_lo[1]), p.act_hi[1]);
    float nlx = lx + ax * h, nly = ly + ay * h;
    lx = fminf(fmaxf(nlx, p.light_lo[0]), p.light_hi[0]);
    ly = fminf(fmaxf(nly, p.light_lo[1]), p.light_hi[1]);
}
// Light.step of every component of the general model: light.py:59-75 (positional), 300-316 (momentum), 237-253 (gradient);
// la = this env's action (ladim floats)
template <class AR>
__device__ __forceinline__ void kb_light_general_step(const AR &p, const float *la, float h, float (&glx)[KB_MAX_LIGHTS],
                                                      float (&gly)[KB_MAX_LIGHTS], float (&glvx)[KB_MAX_LIGHTS], float (&glvy)[KB_MAX_LIGHTS]) {
    if (p.light_type == KB_LIGHT_GRADIENT) {
        const float pi = 3.14159265358979323846f;
        float ang = fminf(fmaxf(la[0], -2.0f * pi), 2.0f * pi);
        if (ang < -pi) ang += 2.0f * pi;
        if (ang > pi) ang -= 2.0f * pi;
        glx[0] = ang;
    } else {
#pragma unroll
        for (int i = 0; i < KB_MAX_LIGHTS; ++i) {
            if (i >= p.lcount) break;
            const float ax = fminf(fmaxf(la[2 * i + 0], p.lalo[i][0]), p.lahi[i][0]);
            const float ay = fminf(fmaxf(la[2 * i + 1], p.lalo[i][1]), p.lahi[i][1]);
            float nlx, nly;
            if (p.lkind[i] == KB_LIGHT_MOMENTUM) {
                float mvx = glvx[i] + ax * h, mvy = glvy[i] + ay * h;
                const float nv = sqrtf(mvx * mvx + mvy * mvy);
                if (nv > p.lmaxv[i]) { const float sc = p.lmaxv[i] / nv; mvx *= sc; mvy *= sc; }
                glvx[i] = mvx; glvy[i] = mvy;
                nlx = glx[i] + mvx * h; nly = gly[i] + mvy * h;
            } else {
                nlx = glx[i] + ax * h; nly = gly[i] + ay * h;
            }
            glx[i] = fminf(fmaxf(nlx, p.llo[i][0]), p.lhi[i][0]);
            gly[i] = fminf(fmaxf(nly, p.llo[i][1]), p.lhi[i][1]);
        }
    }
}
// value_and_gradients of the general model at one sensor position (metres): light.py:176-189, 137-141;
// GradientLight: projection on the gradient direction (intent of light.py:255-260)
template <class AR>
__device__ __forceinline__ void kb_light_general_sense(const AR &p, const float (&glx)[KB_MAX_LIGHTS], const float (&gly)[KB_MAX_LIGHTS],
                                                       float sx, float sy, float &val, float &gx, float &gy) {
    if (p.light_type == KB_LIGHT_GRADIENT) {
        float s_, c_;
        kb_sincosf(glx[0], s_, c_);
        val = c_ * sx + s_ * sy; gx = c_; gy = s_;
        return;
    }
    float vsum = 0.0f, vbest = 0.0f, bgx = 0.0f, bgy = 0.0f;
#pragma unroll
    for (int i = 0; i < KB_MAX_LIGHTS; ++i) {
        if (i >= p.lcount) break;
        float v, x, y;
        kb_light_circular(sx, sy, glx[i], gly[i], p.lradius[i], v, x, y);
        vsum = i == 0 ? v : vsum + v;
        if (i == 0 || v > vbest) { vbest = v; bgx = x; bgy = y; }   // np.argmax: first maximum
    }
    val = vsum; gx = bgx; gy = bgy;
}

// Kilobot.step motor law, kilobot.py:86-127; body velocity in world units
__device__ __forceinline__ void kb_motor_law(int ml, int mr, float th, float h, float &vx, float &vy, float &w) {
    const float max_lin = 0.01f, max_ang = 0.5f * 3.14159265358979323846f;
    float s, c;
    kb_sincosf(th, s, c);
    if (ml && mr) {  // kilobot.py:97-101 (intended meaning; the reference raises TypeError at :127)
        float lin = (float)(mr + ml) / 510.0f * max_lin;
        vx = (s * lin) * WORLD_SCALE; vy = (c * lin) * WORLD_SCALE;
        w = (float)(mr - ml) / 510.0f * max_ang;
    } else if (mr || ml) {  // kilobot.py:103-121: pivot about the opposite leg
        float av, lx, ly = -0.009f;
        if (mr) { av = (float)mr / 255.0f * max_ang; lx = -0.013f; }
        else { av = -(float)ml / 255.0f * max_ang; lx = 0.013f; }
        float ds, dc;
        kb_sincosf(av * h, ds, dc);
        float tx = lx - (dc * lx - ds * ly), ty = ly - (ds * lx + dc * ly);
        tx *= WORLD_SCALE; ty *= WORLD_SCALE;
        float wx = c * tx - s * ty, wy = s * tx + c * ty;  // b2Body::GetWorldVector
        wx = wx / WORLD_SCALE / h; wy = wy / WORLD_SCALE / h;
        vx = wx * WORLD_SCALE; vy = wy * WORLD_SCALE; w = av;
    } else {
        vx = 0.0f; vy = 0.0f; w = 0.0f;
    }
}

__device__ __forceinline__ float kb_clampf(float a, float lo, float hi) { return fmaxf(lo, fminf(a, hi)); }

// ---- x/y pairs of the register solver (kb_regsolve_bins.inc) -----------------------------------
// A two-float vector: component-wise *, + and - on it are v_pk_mul_f32 / v_pk_add_f32, which hold the vector pipe as long as
// one v_mul_f32 (tools/pk_issue_probe.hip).  Every component is rounded exactly as by the scalar instruction, a
// product and the sum behind it stay two operations (-ffp-contract=off, and no helper here fuses them), and a - b * c is the
// subtraction of the rounded product: the same bits as the scalar sequence, signed zeros included.
typedef float kb_pair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ kb_pair pk_load(const float2 &p) { return kb_pair{p.x, p.y}; }      // from the float2 body arrays
__device__ __forceinline__ float2 pk_store(const kb_pair v) { return make_float2(v.x, v.y); }  // ... and back
__device__ __forceinline__ kb_pair pk_splat(const float s) { return kb_pair{s, s}; }
__device__ __forceinline__ float pk_dot(const kb_pair a, const kb_pair b) { const kb_pair t = a * b; return t.x + t.y; }   // a.x * b.x + a.y * b.y
__device__ __forceinline__ kb_pair pk_neg(const kb_pair a) { return -a; }

// LDS operations of one wave execute in program order; this only stops the compiler from moving
// LDS accesses across the point where other lanes' results are consumed.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Read of an LDS word that other waves update with atomics (the union-find parents).  NOTE: through a generic pointer a `volatile`
// access is a FLAT load with system-coherence bits and a full `s_waitcnt vmcnt(0) lgkmcnt(0)` behind it, not a ds_read_b32 (seen
// in the label and flatten passes).  Three ways to get the ds_read were tried in round 3 (a relaxed __hip_atomic_load, a volatile
// access through an LDS-qualified pointer, the same via the low half of the address): each made hipcc 7.2 fail in some OTHER
// instantiation with "Illegal instruction detected: Operand has incorrect register class. V_CMP_NE_U32_e32 0, $src_shared_base",
// so the flat form stays; it was worth ~ 0.5 % of a cfg3 launch.
// A fourth form, a plain load between two compiler barriers (`asm volatile("" ::: "memory"); unsigned v = *p_;
// asm volatile("" : "+v"(v) :: "memory");`), gives the ds_read_b32 in the fixed-size kernels of kb_inst_d0, and fails in
// kb_inst_d2.hip with the same message: "error: Illegal instruction detected: Operand has incorrect register class.
// V_CMP_NE_U32_e32 0, $src_shared_base, implicit-def $vcc, implicit $exec".
// A fifth form, DS_ATOMIC = true: a returning LDS atomic that changes nothing, `atomicOr(p, 0u)`.  The compiler turns it into
// ds_read_b32 + s_waitcnt lgkmcnt(0) -- no FLAT instruction, nothing on the vector-memory counter, and two of them to different
// words go out back to back under one wait.  Used everywhere it fails like the others (kb_inst_d2.hip, same message), so the
// caller selects it per instantiation: the step kernel takes it in the fixed-size sorted-bin kernels only (FN != 0 && BINS,
// all of them in kb_inst_d0.hip, where it compiles); every other instantiation keeps the volatile form.
template <bool DS_ATOMIC = false>
__device__ __forceinline__ unsigned lds_load_relaxed(const unsigned *p_) {
    if constexpr (DS_ATOMIC) return atomicOr(const_cast<unsigned *>(p_), 0u);
    else return *reinterpret_cast<const volatile unsigned *>(p_);
}

// Workgroup barrier for phases that only exchange LDS data: __syncthreads() may also drain the vector-memory counter
// (s_waitcnt vmcnt(0): whenever the compiler sees accesses in flight that its fence has to order), i.e. wait for every
// global load a thread has in flight -- which is exactly what a sweep that requests its records several rounds ahead must
// not do.  Data that changes hands through GLOBAL memory takes __syncthreads() (kb_coopsolve_bins.inc, StoreImpulses).
// No memory instruction inside: the compiler's own s_waitcnt bookkeeping for the registers of outstanding loads stays valid.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- wave-wide reductions / scan over all 64 lanes with DPP (data-parallel primitives: row shifts inside the four rows of
// 16 lanes, then the row_bcast steps across rows): six VALU instructions with no trip to the LDS crossbar, where a
// __shfl_xor / __shfl_up ladder is six dependent ds_bpermute round trips.  All 64 lanes must be active.
#define KB_DPP(v, ctrl, rows) __builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rows, 0xf, true)
__device__ __forceinline__ unsigned wave_or(unsigned v) {       // OR of v over the wave, the same value in every lane
    v |= (unsigned)KB_DPP(v, 0x111, 0xf);      // row_shr:1
    v |= (unsigned)KB_DPP(v, 0x112, 0xf);      // row_shr:2
    v |= (unsigned)KB_DPP(v, 0x114, 0xf);      // row_shr:4
    v |= (unsigned)KB_DPP(v, 0x118, 0xf);      // row_shr:8   -> lane 15 of each row holds its row
    v |= (unsigned)KB_DPP(v, 0x142, 0xa);      // row_bcast:15 into rows 1 and 3
    v |= (unsigned)KB_DPP(v, 0x143, 0xc);      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
    v = max(v, (unsigned)KB_DPP(v, 0x111, 0xf));
    v = max(v, (unsigned)KB_DPP(v, 0x112, 0xf));
    v = max(v, (unsigned)KB_DPP(v, 0x114, 0xf));
    v = max(v, (unsigned)KB_DPP(v, 0x118, 0xf));
    v = max(v, (unsigned)KB_DPP(v, 0x142, 0xa));
    v = max(v, (unsigned)KB_DPP(v, 0x143, 0xc));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {   // inclusive prefix sum over the lanes
    v += (unsigned)KB_DPP(v, 0x111, 0xf);
    v += (unsigned)KB_DPP(v, 0x112, 0xf);
    v += (unsigned)KB_DPP(v, 0x114, 0xf);
    v += (unsigned)KB_DPP(v, 0x118, 0xf);
    v += (unsigned)KB_DPP(v, 0x142, 0xa);
    v += (unsigned)KB_DPP(v, 0x143, 0xc);
    return v;
}

// What the solvers and the continuous step read of the kernel arguments, as a copy a phase makes at its head (kb_step_kernel.h:
// phase-scoped arguments) -- so that no sweep and no event loop carries a scalar load: the arena for wall_geom, and the
// constants of the contact arithmetic.
struct SolveArgs {
    float xmin, ymin, xmax, ymax, h;
    int vel_iters, pos_iters, exact_div;
    float im_bot, r_bot, nm_bb, nm_wb, y_bb, y_wb;
};
template <class AR>
__device__ __forceinline__ SolveArgs solve_args(const AR &p) {
    return {p.xmin, p.ymin, p.xmax, p.ymax, p.h, p.vel_iters, p.pos_iters, p.exact_div, p.im_bot, p.r_bot, p.nm_bb, p.nm_wb, p.y_bb, p.y_wb};
}

template <class AR>
__device__ __forceinline__ void wall_geom(const AR &p, int wl, float x, float y, float &dist, float &nx, float &ny) {
    switch (wl) {
    case 0: nx = 1.0f; ny = 0.0f; dist = x - p.xmin; break;
    case 1: nx = 0.0f; ny = 1.0f; dist = y - p.ymin; break;
    case 2: nx = -1.0f; ny = 0.0f; dist = p.xmax - x; break;
    default: nx = 0.0f; ny = -1.0f; dist = p.ymax - y; break;
    }
}

#ifdef KB_PROFILE
// diagnostic build: thread 0 accumulates shader cycles per phase into g.status[E + 8*e + phase]
// (light-weight: one 32-bit time register and fire-and-forget LDS atomics on the free words 24.. of the misc area; the first
//  version kept 24 64-bit accumulators in registers, which the allocator spilled: every stamp was a scratch round trip and a
//  fifth of the profiled time was the profile itself)
#define KB_PROF(k) misc[24 + (k)]
#define KB_STAMP(ph) do { if (tid == 0) { const unsigned t_ = (unsigned)clock64(); atomicAdd(&KB_PROF(ph), t_ - prof_t); prof_t = t_; } } while (0)
// time since the last stamp without closing the interval: wave 0's own work before it waits at the barrier
#define KB_STAMP_PRE(ph) do { if (tid == 0) { atomicAdd(&KB_PROF(ph), (unsigned)clock64() - prof_t); } } while (0)
#else
#define KB_STAMP(ph) do { } while (0)
#define KB_STAMP_PRE(ph) do { } while (0)
#endif

// b2TimeOfImpact for a circle (radius R) whose centre moves linearly from (x0,y0) to (x1,y1) against wall wl:
// Box2D's control flow (conservative advancement + bisection / secant root finder) on the closed-form distance of
// the centre to an axis-aligned wall.  True and t in [0,1] when the state is e_touching.
template <class AR>
__device__ __forceinline__ bool kb_toi_wall(const AR &p, int wl, float R, float x0, float y0, float x1, float y1, float &tout) {
    const float total = R + B2_POLYGON_RADIUS;
    const float target = fmaxf(B2_LINEAR_SLOP, total - 3.0f * B2_LINEAR_SLOP);
    const float tol = 0.25f * B2_LINEAR_SLOP;
    float nx, ny;
    auto dist_at = [&](float t) __attribute__((always_inline)) -> float {
        float dv;
        wall_geom(p, wl, (1.0f - t) * x0 + t * x1, (1.0f - t) * y0 + t * y1, dv, nx, ny);
        return dv;
    };
    float t1 = 0.0f;
    for (int iter = 0; iter < 20; ++iter) {
        const float dist = dist_at(t1);
        if (fabsf(dist) <= 0.0f) return false;                        // overlapped
        if (fabsf(dist) < target + tol) { tout = t1; return true; }   // touching
        float t2 = 1.0f;
        for (int push = 0; push < 8; ++push) {
            float s2 = dist_at(t2);
            if (s2 > target + tol) return false;                      // separated at the end of the step
            if (s2 > target - tol) { t1 = t2; break; }
            float s1 = dist_at(t1);
            if (s1 < target - tol) return false;                      // failed
            if (s1 <= target + tol) { tout = t1; return true; }
            float a1 = t1, a2 = t2;
            for (int root = 0; root < 50; ++root) {                   // bisection / secant alternating
                const float t = (root & 1) ? a1 + (target - s1) * (a2 - a1) / (s2 - s1) : 0.5f * (a1 + a2);
                const float sv = dist_at(t);
                if (fabsf(sv - target) < tol) { t2 = t; break; }
                if (sv > target) { a1 = t; s1 = sv; } else { a2 = t; s2 = sv; }
            }
        }
    }
    return false;                                                     // failed (iteration cap)
}

// The first iteration of kb_toi_wall for the sweep (x0,y0) -> (x1,y1) against wall wl and nothing more: d0 = dist_at(0) and
// d1 = dist_at(1) by the same expressions, tt = target + tol by the same operations (Params::toi_tt for a kilobot).
// True: kb_toi_wall returns false for this sweep.  It returns true along two ways only -- |d0| < tt (touching at the start),
// or from inside the push loop, which it leaves with false at once when d1 > tt -- and d0 == 0 is "overlapped", false.
// The negation stays as written: an unordered compare keeps the body a candidate.
// A body for which this holds on all four walls goes through kb_toi_walls_body unchanged: minAlpha stays 1 and the event
// loop breaks in front of its first change; later events need a first one, whose sweep is this one.
template <class AR>
__device__ __forceinline__ bool kb_toi_no_event(const AR &p, int wl, float tt, float x0, float y0, float x1, float y1) {
    float d0, d1, nx, ny;
    wall_geom(p, wl, (1.0f - 0.0f) * x0 + 0.0f * x1, (1.0f - 0.0f) * y0 + 0.0f * y1, d0, nx, ny);
    wall_geom(p, wl, (1.0f - 1.0f) * x0 + 1.0f * x1, (1.0f - 1.0f) * y0 + 1.0f * y1, d1, nx, ny);
    return fabsf(d0) <= 0.0f || (!(fabsf(d0) < tt) && d1 > tt);
}

// b2World::SolveTOI + b2Island::SolveTOI for one circular body against the arena walls (the only TOI events Box2D
// computes for non-bullet bodies).  (x0,y0,a0): pose at the start of the step; (x,y,a): pose after b2Island::Solve;
// (vx,vy,w): velocity after the solve; updated in place.
template <class AR>
__device__ __forceinline__ void kb_toi_walls_body(const AR &p, float R, float im, float x0, float y0, float a0,
                                                  float &x, float &y, float &a, float &vx, float &vy, float &w) {
    const float h = p.h;
    const float total = R + B2_POLYGON_RADIUS;
    // quick reject: a body that stays clear of every wall by more than its contact radius has no TOI event
    {
        const float m0 = fminf(fminf(x0 - p.xmin, p.xmax - x0), fminf(y0 - p.ymin, p.ymax - y0));
        const float m1 = fminf(fminf(x - p.xmin, p.xmax - x), fminf(y - p.ymin, p.ymax - y));
        if (m0 > total && m1 > total) return;
    }
    float alpha0 = 0.0f;
    float c0x = x0, c0y = y0, ca0 = a0, cx = x, cy = y, ca = a;
    for (int ev = 0; ev < B2_MAX_SUBSTEPS; ++ev) {
        float minAlpha = 1.0f;
#pragma unroll
        for (int wl = 0; wl < 4; ++wl) {
            float t;
            float alpha = 1.0f;
            if (kb_toi_wall(p, wl, R, c0x, c0y, cx, cy, t)) alpha = fminf(alpha0 + (1.0f - alpha0) * t, 1.0f);
            if (alpha < minAlpha) minAlpha = alpha;
        }
        if (1.0f - 10.0f * B2_EPSILON < minAlpha) break;
        const float beta = (minAlpha - alpha0) / (1.0f - alpha0);      // b2Body::Advance
        c0x += beta * (cx - c0x); c0y += beta * (cy - c0y); ca0 += beta * (ca - ca0);
        alpha0 = minAlpha;
        cx = c0x; cy = c0y; ca = ca0;
        bool touch[4];
        float wnx[4], wny[4];
#pragma unroll
        for (int wl = 0; wl < 4; ++wl) {                               // manifolds of the static contacts at the TOI pose
            float dist;
            wall_geom(p, wl, cx, cy, dist, wnx[wl], wny[wl]);
            touch[wl] = !(dist * dist > total * total);
            if (dist < 0.0f) { wnx[wl] = -wnx[wl]; wny[wl] = -wny[wl]; }
        }
        for (int it = 0; it < 20; ++it) {                              // SolveTOIPositionConstraints
            float minSep = 0.0f;
#pragma unroll
            for (int wl = 0; wl < 4; ++wl) {
                if (!touch[wl]) continue;
                float dist, bx, by;
                wall_geom(p, wl, cx, cy, dist, bx, by);
                const float along = (wnx[wl] == bx && wny[wl] == by) ? dist : -dist;
                const float sep = along - B2_POLYGON_RADIUS - R;
                minSep = fminf(minSep, sep);
                const float C = kb_clampf(B2_TOI_BAUMGARTE * (sep + B2_LINEAR_SLOP), -B2_MAX_LINEAR_CORRECTION, 0.0f);
                const float K = 0.0f + im;
                const float imp = K > 0.0f ? -C / K : 0.0f;
                cx += im * (imp * wnx[wl]); cy += im * (imp * wny[wl]);
            }
            if (minSep >= -1.5f * B2_LINEAR_SLOP) break;
        }
        c0x = cx; c0y = cy; ca0 = ca;                                   // leap of faith to the new safe state
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int it = 0; it < p.vel_iters; ++it) {                      // velocity constraints, no warm starting
#pragma unroll
            for (int wl = 0; wl < 4; ++wl) {
                if (!touch[wl]) continue;
                const float vn = vx * wnx[wl] + vy * wny[wl];
                const float k = 0.0f + im;
                const float nm = k > 0.0f ? 1.0f / k : 0.0f;
                float lambda = -(nm * vn);
                const float newimp = fmaxf(acc[wl] + lambda, 0.0f);
                lambda = newimp - acc[wl];
                acc[wl] = newimp;
                vx += im * (lambda * wnx[wl]); vy += im * (lambda * wny[wl]);
            }
        }
        const float hh = (1.0f - minAlpha) * h;                         // integrate the rest of the step
        const float tx = hh * vx, ty = hh * vy;
        if (tx * tx + ty * ty > B2_MAX_TRANSLATION_SQ) {
            const float ratio = B2_MAX_TRANSLATION / sqrtf(tx * tx + ty * ty);
            vx *= ratio; vy *= ratio;
        }
        const float rot = hh * w;
        if (rot * rot > B2_MAX_ROTATION_SQ) w *= B2_MAX_ROTATION / fabsf(rot);
        cx += hh * vx; cy += hh * vy; ca += hh * w;
    }
    x = cx; y = cy; a = ca;
}

// atomic exchange on a 16-bit LDS cell (LDS atomics are 32-bit: compare-and-swap on the containing word)
__device__ __forceinline__ unsigned kb_exch16(unsigned short *base, int idx, unsigned val) {
    unsigned *word = reinterpret_cast<unsigned *>(base) + (idx >> 1);
    const int sh = (idx & 1) * 16;
    unsigned old = lds_load_relaxed(word);
    for (;;) {
        const unsigned want = (old & ~(0xFFFFu << sh)) | (val << sh);
        const unsigned seen = atomicCAS(word, old, want);
        if (seen == old) break;
        old = seen;
    }
    return (old >> sh) & 0xFFFFu;
}

// IR-range neighbour sensing off the cell lists of the broadphase: kilobot a walks the half stencil of reach s
// (own cell: partners with a higher id; the cells to the east in its row; every cell of the s rows above), so that every
// pair is met exactly once, and both ends of a pair within range are counted.  cnt16: u16 counters packed in pairs
// (LDS atomics are 32-bit; a count is at most N - 1 < 65536, so no carry crosses the halves); zeroed by the caller.
// Out of line: the kernels that never sense do not pay registers for it.
__device__ __noinline__ void kb_sense_pass(const float2 *pos, const unsigned short *head, const unsigned short *nextb,
                                           const unsigned short *cellOf, unsigned *cnt16, int N, int nt, int tid,
                                           int gw, int gh, int s, float R2, int hmask) {
    constexpr int W = 8;      // list heads fetched together (one LDS round trip); most cells are empty
    for (int a = tid; a < N; a += nt) {
        const int cell = cellOf[a];
        const int cx = cell % gw, cy = cell / gw;
        const float2 pa = pos[a];
        unsigned mine = 0;
        for (int dy = 0; dy <= s; ++dy) {
            const int oy = cy + dy;
            if (oy >= gh) break;
            const int x0 = dy == 0 ? cx : max(cx - s, 0), x1 = min(cx + s, gw - 1);
            for (int xb = x0; xb <= x1; xb += W) {
                unsigned cur[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {      // (hmask: the heads are a hash table of the cells, the walk checks the candidate's cell)
                    const int c_ = oy * gw + xb + i;
                    cur[i] = xb + i <= x1 ? (unsigned)head[hmask ? (c_ & hmask) : c_] : (unsigned)EMPTY16;
                }
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const bool own = dy == 0 && xb + i == cx;
                    for (unsigned b = cur[i]; b != (unsigned)EMPTY16;) {
                        const float2 pb = pos[b];
                        const unsigned nb = nextb[b];
                        if (!(own && (int)b <= a) && (!hmask || (int)cellOf[b] == oy * gw + xb + i)) {
                            const float ex = pb.x - pa.x, ey = pb.y - pa.y;
                            const float dd = ex * ex + ey * ey;
                            if (!(dd > R2)) {
                                mine++;
                                atomicAdd(&cnt16[b >> 1], 1u << (16 * (b & 1u)));
                            }
                        }
                        b = nb;
                    }
                }
            }
        }
        if (mine) atomicAdd(&cnt16[a >> 1], mine << (16 * (a & 1)));
    }
}

// ---- counter-based random numbers for kb_reset: Philox4x32-10 (Salmon et al., SC'11), Cephes logf ------------------
struct U4 { unsigned x, y, z, w; };
__host__ __device__ inline unsigned kb_mulhi32(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * (unsigned long long)b) >> 32); }
__host__ __device__ inline U4 kb_philox4x32_10(U4 c, unsigned k0, unsigned k1) {
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = kb_mulhi32(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = kb_mulhi32(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        U4 n;
        n.x = hi1 ^ c.y ^ k0; n.y = lo1; n.z = hi0 ^ c.w ^ k1; n.w = lo0;
        c = n;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}
// natural logarithm of a positive normal float: Cephes single-precision algorithm (frexp by bit manipulation, degree-8
// minimax polynomial); own implementation so that the device and the oracle give the same bits.
__device__ __forceinline__ float kb_logf(float xx) {
    unsigned bits = __float_as_uint(xx);
    int e = (int)((bits >> 23) & 255u) - 126;
    float x = __uint_as_float((bits & 0x807FFFFFu) | 0x3F000000u);     // mantissa in [0.5, 1)
    if (x < 0.707106781186547524f) { e -= 1; x = x + x - 1.0f; }
    else x = x - 1.0f;
    float z = x * x;
    float y = ((((((((7.0376836292E-2f * x - 1.1514610310E-1f) * x + 1.1676998740E-1f) * x - 1.2420140846E-1f) * x
                  + 1.4249322787E-1f) * x - 1.6668057665E-1f) * x + 2.0000714765E-1f) * x - 2.4999993993E-1f) * x
               + 3.3333331174E-1f) * x * z;
    const float fe = (float)e;
    if (e) y += -2.12194440e-4f * fe;
    y += -0.5f * z;
    z = x + y;
    if (e) z += 0.693359375f * fe;
    return z;
}

__device__ __forceinline__ int dir_dx(int k) { return (k == 1 || k == 3) ? 1 : (k == 4 ? -1 : 0); }
__device__ __forceinline__ int dir_dy(int k) { return (k >= 2) ? 1 : 0; }

// exclusive scan of NP (multiple of 4, <= 4 * blockDim.x) u8 counts into u16 offsets; returns the total.
// All threads must call; contains two workgroup barriers.
// (tid: the caller's copy of threadIdx.x -- inside the substep loop an opaque one, so that nothing derived from it is hoisted
//  out of the loop and kept in spilled registers)
__device__ __forceinline__ unsigned block_scan_u8(const unsigned char *cnt, unsigned short *off, int NP, unsigned *wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const bool in = 4 * tid < NP;
    const unsigned c4 = in ? *reinterpret_cast<const unsigned *>(cnt + 4 * tid) : 0u;
    const unsigned c0 = c4 & 255u, c1 = (c4 >> 8) & 255u, c2 = (c4 >> 16) & 255u, c3 = c4 >> 24;
    const unsigned sum = c0 + c1 + c2 + c3;
    const unsigned incl = wave_incl_scan(sum);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned base = 0, total = 0;
    for (int w = 0; w < nw; ++w) { const unsigned s = wsum[w]; if (w < wave) base += s; total += s; }
    if (in) {
        const unsigned r0 = base + incl - sum, r1 = r0 + c0, r2 = r1 + c1, r3 = r2 + c2;
        reinterpret_cast<unsigned *>(off + 4 * tid)[0] = r0 | (r1 << 16);
        reinterpret_cast<unsigned *>(off + 4 * tid)[1] = r2 | (r3 << 16);
    }
    __syncthreads();
    return total;
}



// ---- sorted bins: inclusive scan of the bin counters ------------------------------------------------------------------
// E1[0] = 0, E1[i] (i >= 1) = kilobots counted into bin i - 1; afterwards E1[i] = kilobots in bins < i, i.e. bin b occupies the
// slots [E1[b], E1[b + 1]).  nchunks chunks of 8 u16 entries (16 bytes, padding zero); thread t scans `per` consecutive chunks.
// All threads must call; two workgroup barriers inside.
template <bool ONE>
__device__ __forceinline__ void block_scan_bins(unsigned short *E1, int nchunks, int per, unsigned *wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int c0 = ONE ? tid : tid * per, c1 = ONE ? min(tid + 1, nchunks) : min(c0 + per, nchunks);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    unsigned sum = 0;
    for (int c = c0; c < c1; ++c) {
        v = reinterpret_cast<const uint4 *>(E1)[c];
        sum += (v.x & 0xFFFFu) + (v.x >> 16) + (v.y & 0xFFFFu) + (v.y >> 16) + (v.z & 0xFFFFu) + (v.z >> 16) + (v.w & 0xFFFFu) + (v.w >> 16);
    }
    const unsigned incl = wave_incl_scan(sum);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (int w = 0; w < nw; ++w) { const unsigned s = wsum[w]; if (w < wave) run += s; }
    for (int c = c0; c < c1; ++c) {
        if (!ONE) v = reinterpret_cast<const uint4 *>(E1)[c];
        uint4 o;
        unsigned a, b;
        a = run + (v.x & 0xFFFFu); b = a + (v.x >> 16); o.x = a | (b << 16);
        a = b + (v.y & 0xFFFFu); b = a + (v.y >> 16); o.y = a | (b << 16);
        a = b + (v.z & 0xFFFFu); b = a + (v.z >> 16); o.z = a | (b << 16);
        a = b + (v.w & 0xFFFFu); b = a + (v.w >> 16); o.w = a | (b << 16);
        run = b;
        reinterpret_cast<uint4 *>(E1)[c] = o;
    }
    __syncthreads();
}

// IR-range neighbour sensing off the sorted bins (arena-sized grid, no hashing): the kilobots of the cells x0 .. x1 of a
// grid row are ONE run of slots, two loads per row.  Slot sa walks the half stencil of reach s (its own row: the slots
// behind it up to the end of cell cx + s; the s rows above: cells cx - s .. cx + s), meets every pair once and counts
// both ends.  cnt16: u16 counters per slot packed in pairs (zeroed by the caller).
__device__ __noinline__ void kb_sense_bins(const float2 *pos, const unsigned short *E1, unsigned *cnt16, int sa, int cx, int cy,
                                           int gw, int gh, int s, float R2) {
    const float2 pa = pos[sa];
    unsigned mine = 0;
    for (int dy = 0; dy <= s; ++dy) {
        const int oy = cy + dy;
        if (oy >= gh) break;
        const int x0 = max(cx - s, 0), x1 = min(cx + s, gw - 1);
        int lo = dy == 0 ? sa + 1 : (int)E1[oy * gw + x0];
        const int hi = (int)E1[oy * gw + x1 + 1];
        for (int b = lo; b < hi; ++b) {
            const float2 pb = pos[b];
            const float ex = pb.x - pa.x, ey = pb.y - pa.y;
            const float dd = ex * ex + ey * ey;
            if (!(dd > R2)) {
                mine++;
                atomicAdd(&cnt16[b >> 1], 1u << (16 * (b & 1)));
            }
        }
    }
    if (mine) atomicAdd(&cnt16[sa >> 1], mine << (16 * (sa & 1)));
}
// the same over hashed bins (sparse swarms): cell by cell, every candidate checked against the cell it must be in
__device__ __noinline__ void kb_sense_bins_hashed(const float2 *pos, const unsigned short *E1, const unsigned short *cellOfSlot, unsigned *cnt16,
                                                  int sa, int cx, int cy, int gw, int gh, int s, float R2, int hmask) {
    const float2 pa = pos[sa];
    unsigned mine = 0;
    for (int dy = 0; dy <= s; ++dy) {
        const int oy = cy + dy;
        if (oy >= gh) break;
        const int x0 = dy == 0 ? cx : max(cx - s, 0), x1 = min(cx + s, gw - 1);
        for (int ox = x0; ox <= x1; ++ox) {
            const int cell = oy * gw + ox, bin = cell & hmask;
            const bool own = dy == 0 && ox == cx;
            const int lo = own ? sa + 1 : (int)E1[bin], hi = (int)E1[bin + 1];
            for (int b = lo; b < hi; ++b) {
                if ((int)cellOfSlot[b] != cell) continue;
                const float2 pb = pos[b];
                const float ex = pb.x - pa.x, ey = pb.y - pa.y;
                const float dd = ex * ex + ey * ey;
                if (!(dd > R2)) {
                    mine++;
                    atomicAdd(&cnt16[b >> 1], 1u << (16 * (b & 1)));
                }
            }
        }
    }
    if (mine) atomicAdd(&cnt16[sa >> 1], mine << (16 * (sa & 1)));
}

typedef void (*kb_step_fn)(const Params);
// kb_step_kernel<kb_variants.v[i]> at [i], entered by the kb_inst_*.hip units that instantiate it (kb_step_kernel.h:
// register_unit), nullptr where no linked unit does (kb_abi.hip)
extern kb_step_fn kb_kernels[NUM_VARIANTS];

}  // namespace kb
