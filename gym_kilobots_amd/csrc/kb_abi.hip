// kb_abi.hip -- the C ABI of libkilobots_hip.so (include/kilobots_hip.h): argument validation and launches of every entry
// point, kb_create's derivation of the kernel parameters (Params: grid, masses, damping, object and light tables) from a
// kb_config, and the small kernels that need no LDS image: set_actions, the pose / state read-backs, kb_reset's spawn and
// kb_light_sense.  The sensing kernels (kb_sense, kb_sense_neighbors, kb_sense_histogram, kb_sense_reduce, kb_sense_objects,
// kb_sense_grid, kb_sense_contacts, kb_sense_rays, kb_sense_edges, kb_sense_hops, kb_sense_clusters, kb_sense_coverage, kb_sense_targets, kb_sense_assign, kb_field_step, kb_sense_paths) and the rasteriser of kb_render are in kb_sense.h.
//
// The hot kernel is kb_step_kernel (kb_step_kernel.h, instantiated per drive law in kb_inst_*.hip, picked by kb_variant.h):
// one workgroup owns one env for the whole launch: poses are loaded once from HBM into LDS, `n_substeps` iterations
// of the reference substep loop (gym_kilobots/envs/kilobots_env.py:168-190) run out of LDS / registers, poses are
// written back once.  Per substep:
//   drive law (kilobot.py:86-127,191-203,253-258,294-300,318-333) + light (light.py:59-75,99-148,176-189,218-319)
//   -> broadphase: uniform grid of per-cell linked lists in LDS (one atomic exchange per bot)
//   -> narrowphase: circle-circle / circle-wall / circle-polygon (Box2D b2CollideCircles, b2CollideEdgeAndCircle,
//      b2CollidePolygonAndCircle), 5-cell half stencil, warm-start impulses matched from the previous substep;
//      manifolds of the object-object and object-wall contacts (kb_objects.h)
//   -> islands: lock-free union-find in LDS; islands placed on wavefronts in order of size
//   -> solver (b2ContactSolver semantics): warm start + 10 sequential-impulse velocity sweeps, symplectic Euler,
//      <= 10 position sweeps with Box2D's per-island early out, continuous step against the walls.
// Gauss-Seidel order.  Every contact gets a key (class, rank): class from the relative grid position of the two
// bodies and the parity of the base cell, rank from its position inside its cell-pair group.  Two contacts with the
// same key never share a body, so all contacts of one key can be solved concurrently and the result equals the
// sequential sweep in (class, group, A, B) order that DESIGN.md specifies.  Islands are independent, so each island
// is bound to ONE wavefront, which sweeps its contacts level by level of their dependency depth with no workgroup
// barrier at all (LDS operations of one wave execute in order).  Only when one island is very large does the whole
// workgroup cooperate on the sweep with s_barrier between keys.
// No MFMA anywhere: this is LDS-, issue- and HBM-bound integer/float work.
//
// Arithmetic: fp32, compiled with -ffp-contract=off; every expression is written in the operation order of the
// specification so results do not depend on launch fusion, workgroup size or sharding.
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "kb_common.h"
#include "kb_objects.h"
#include "kb_sense.h"

using namespace kb;

namespace {

// set_action alone (kilobot.py:235-241, 283-289)
__global__ void kb_set_actions_kernel(const Params p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t T = (size_t)p.E * p.N;
    if (i >= T) return;
    float a0 = 0.0f, a1 = 0.0f;
    if (p.actions) { const float2 a = reinterpret_cast<const float2 *>(p.actions)[i]; a0 = a.x; a1 = a.y; }
    const int law = p.drive_mode == KB_DRIVE_MIXED ? (int)p.buf.bot_mode[i] : p.drive_mode;
    if (law == KB_DRIVE_VELOCITY) {
        const float mw = 0.5f * 3.14159265358979323846f;
        p.buf.v[i] = fmaxf(fminf(a0, 0.01f), 0.0f);
        p.buf.w[i] = fmaxf(fminf(a1, mw), -mw);
    } else if (law == KB_DRIVE_ACCEL) {
        const float aw = 0.2f * 3.14159265358979323846f;
        p.buf.acc_v[i] = fmaxf(fminf(a0, 0.005f), -0.005f);
        p.buf.acc_w[i] = fmaxf(fminf(a1, aw), -aw);
    }
}

// Body.get_pose for every kilobot (body.py:63-65): metres, radians
__global__ void kb_get_poses_kernel(const float *x, const float *y, const float *th, float *out, size_t T) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    out[3 * i + 0] = x[i] / WORLD_SCALE;
    out[3 * i + 1] = y[i] / WORLD_SCALE;
    out[3 * i + 2] = th[i];
}

// KilobotsEnv.get_state() in one read (kilobots_env.py:115-118): per env 3 N kilobot words, 3 M object words, the status word
__global__ void kb_get_state_kernel(const Params p, float *out) {
    const int per = p.N + p.M + 1;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.E * per) return;
    const size_t e = i / per;
    const int k = (int)(i - e * per);
    float *row = out + e * (size_t)(3 * per - 2);
    if (k < p.N) {
        const size_t j = e * p.N + k;
        row[3 * k + 0] = p.buf.x[j] / WORLD_SCALE;
        row[3 * k + 1] = p.buf.y[j] / WORLD_SCALE;
        row[3 * k + 2] = p.buf.theta[j];
    } else if (k < p.N + p.M) {
        const size_t j = e * p.M + (k - p.N);
        row[3 * k + 0] = p.buf.ox[j] / WORLD_SCALE;
        row[3 * k + 1] = p.buf.oy[j] / WORLD_SCALE;
        row[3 * k + 2] = p.buf.otheta[j];
    } else {
        row[3 * k] = __int_as_float(p.buf.status[e]);
    }
}

// The sensing point of a substep on its own (kb_light_sense): light.step + value_and_gradients at every kilobot's sensor
// (kilobots_env.py:171-180), with the arithmetic of the step kernel (shared functions of kb_common.h), for kilobots whose
// _loop runs on the host between the sensing and the motor law.  One workgroup per env.
__global__ void __launch_bounds__(256) kb_light_sense_kernel(const Params p, const float *light_action) {
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const kb_buffers &g = p.buf;
    const size_t o = (size_t)e * N;
    const bool general = p.light_type != KB_LIGHT_CIRCULAR;
    float lx = 0.0f, ly = 0.0f;
    float glx[KB_MAX_LIGHTS], gly[KB_MAX_LIGHTS], glvx[KB_MAX_LIGHTS], glvy[KB_MAX_LIGHTS];
#pragma unroll
    for (int i = 0; i < KB_MAX_LIGHTS; ++i) { glx[i] = 0.0f; gly[i] = 0.0f; glvx[i] = 0.0f; glvy[i] = 0.0f; }
    if (!general) { lx = g.light_x[e]; ly = g.light_y[e]; }
    else {
#pragma unroll
        for (int i = 0; i < KB_MAX_LIGHTS; ++i) {
            if (i >= p.lcount) break;
            glx[i] = g.light_x[(size_t)e * p.lcount + i];
            if (p.light_type != KB_LIGHT_GRADIENT) gly[i] = g.light_y[(size_t)e * p.lcount + i];
            if (p.lkind[i] == KB_LIGHT_MOMENTUM) { glvx[i] = g.light_vx[(size_t)e * p.lcount + i]; glvy[i] = g.light_vy[(size_t)e * p.lcount + i]; }
        }
    }
    __syncthreads();      // every thread holds the old light state before thread 0 stores the new one
    if (light_action) {
        if (general) kb_light_general_step(p, light_action + (size_t)e * p.ladim, p.h, glx, gly, glvx, glvy);
        else kb_light_single_step(p, light_action + 2 * e, p.h, lx, ly);
        if (tid == 0) {
            if (!general) { g.light_x[e] = lx; g.light_y[e] = ly; }
            else {
#pragma unroll
                for (int i = 0; i < KB_MAX_LIGHTS; ++i) {
                    if (i >= p.lcount) break;
                    g.light_x[(size_t)e * p.lcount + i] = glx[i];
                    if (p.light_type != KB_LIGHT_GRADIENT) g.light_y[(size_t)e * p.lcount + i] = gly[i];
                    if (p.lkind[i] == KB_LIGHT_MOMENTUM) { g.light_vx[(size_t)e * p.lcount + i] = glvx[i]; g.light_vy[(size_t)e * p.lcount + i] = glvy[i]; }
                }
            }
        }
    }
    for (int b = tid; b < N; b += nt) {
        const float bx = g.x[o + b], by = g.y[o + b];
        float sx = bx, sy = by;
        if ((p.drive_mode == KB_DRIVE_MIXED ? (int)g.bot_mode[o + b] : p.drive_mode) != KB_DRIVE_SIMPLE_PHOTOTAXIS) {  // kilobot.py:54-55: world point of (0, -r)
            float s, c;
            kb_sincosf(g.theta[o + b], s, c);
            const float lx0 = 0.0f, ly0 = -p.r_bot;
            sx = (c * lx0 - s * ly0) + bx;
            sy = (s * lx0 + c * ly0) + by;
        }
        float lval, lgx, lgy;
        if (general) kb_light_general_sense(p, glx, gly, sx / WORLD_SCALE, sy / WORLD_SCALE, lval, lgx, lgy);
        else kb_light_circular(sx / WORLD_SCALE, sy / WORLD_SCALE, lx, ly, p.light_radius, lval, lgx, lgy);
        g.light_value[o + b] = lval; g.light_gx[o + b] = lgx; g.light_gy[o + b] = lgy;
    }
}

// KilobotsEnv.reset spawn (kb_reset): one thread per kilobot, Philox4x32-10 keyed by the seed, counter (global env, bot)
struct ResetArgs {
    unsigned k0, k1;
    int env_offset, random_theta, random_velocity;
    float mean_x, mean_y, std, lo_x, lo_y, hi_x, hi_y;
    // kb_reset_envs (all NULL in kb_reset): the envs to reset, word z of their Philox counters, and what to put their objects and lights at
    const unsigned char *env_mask;
    const unsigned *episode;
    const float *obj_pose, *light_pos, *light_vel;
};
__global__ void kb_reset_kernel(const Params p, const ResetArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t T = (size_t)p.E * p.N;
    if (i >= T) return;
    const int e = (int)(i / p.N), b = (int)(i % p.N);
    if (a.env_mask && !a.env_mask[e]) return;
    U4 c;
    c.x = (unsigned)(a.env_offset + e); c.y = (unsigned)b; c.z = a.episode ? a.episode[e] : 0u; c.w = 0u;
    const U4 r = kb_philox4x32_10(c, a.k0, a.k1);
    // Box-Muller on u1 in (0, 1], u2 in [0, 1)
    const float u1 = (float)((r.x >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * kb_logf(u1));
    float sn, cs;
    kb_sincosf(6.28318530717958647692f * u2, sn, cs);
    float xm = a.mean_x + a.std * (rad * cs), ym = a.mean_y + a.std * (rad * sn);
    xm = fminf(fmaxf(xm, a.lo_x), a.hi_x); ym = fminf(fmaxf(ym, a.lo_y), a.hi_y);   // yaml_kilobots_env.py:350-351
    p.buf.x[i] = xm * WORLD_SCALE; p.buf.y[i] = ym * WORLD_SCALE;
    float th = 0.0f;                                                                   // body.py:28-29
    if (a.random_theta) th = ((float)(r.z >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f) * 3.14159265358979323846f;
    p.buf.theta[i] = th;
    p.buf.ws_cnt[i] = 0;
    const int law = p.drive_mode == KB_DRIVE_MIXED ? (int)p.buf.bot_mode[i] : p.drive_mode;
    if (law == KB_DRIVE_VELOCITY || law == KB_DRIVE_ACCEL) {
        float v = 0.0f, w = 0.0f;
        if (a.random_velocity) {                                                       // kilobot.py:225-229
            v = (float)(r.w & 0xFFFFu) * (1.0f / 65536.0f) * 0.01f;
            w = ((float)(r.w >> 16) * (1.0f / 65536.0f) * 2.0f - 1.0f) * (0.5f * 3.14159265358979323846f);
        }
        p.buf.v[i] = v; p.buf.w[i] = w;
    }
    if (law == KB_DRIVE_ACCEL) { p.buf.acc_v[i] = 0.0f; p.buf.acc_w[i] = 0.0f; }
    if (law == KB_DRIVE_MOTORS || law == KB_DRIVE_PHOTOTAXIS) { p.buf.motor_l[i] = 255; p.buf.motor_r[i] = 0; }   // turn_left
    if (law == KB_DRIVE_PHOTOTAXIS) {
        p.buf.pt_threshold[i] = -INFINITY; p.buf.pt_update[i] = 0; p.buf.pt_nochange[i] = 0; p.buf.pt_dir[i] = 0;
    }
    if (b == 0) p.buf.status[e] = 0;
    if (p.buf.sleep_time) p.buf.sleep_time[i] = 0.0f;      // new bodies are awake (b2BodyDef::awake)
    if (p.buf.nbr_count) p.buf.nbr_count[i] = 0u;          // (the resolve step does not sense: no counts of the previous episode)
    if (p.M > 0) {      // forget the objects' manifold impulses as well
        float *ows = p.buf.ows_acc + (size_t)e * (MAXOBJ * KB_OWS_COLS * KB_OWS_WORDS);
        for (int k = b; k < MAXOBJ * KB_OWS_COLS * KB_OWS_WORDS; k += p.N) ows[k] = -1.0f;
    }
    if (a.obj_pose) {   // the env's objects at the caller's poses, at rest and awake (Body.__init__, body.py:32-38)
        for (int k = b; k < p.M; k += p.N) {
            const size_t j = (size_t)e * p.M + k;
            p.buf.ox[j] = a.obj_pose[3 * j + 0]; p.buf.oy[j] = a.obj_pose[3 * j + 1]; p.buf.otheta[j] = a.obj_pose[3 * j + 2];
            p.buf.ovx[j] = 0.0f; p.buf.ovy[j] = 0.0f; p.buf.ow[j] = 0.0f;
            if (p.buf.osleep) p.buf.osleep[j] = 0.0f;
        }
    }
    if (a.light_pos || a.light_vel) {
        for (int k = b; k < p.lcount; k += p.N) {
            const size_t j = (size_t)e * p.lcount + k;
            if (a.light_pos) {
                p.buf.light_x[j] = a.light_pos[2 * j + 0];
                if (p.buf.light_y) p.buf.light_y[j] = a.light_pos[2 * j + 1];
            }
            if (p.buf.light_vx && p.buf.light_vy) {
                p.buf.light_vx[j] = a.light_vel ? a.light_vel[2 * j + 0] : 0.0f;
                p.buf.light_vy[j] = a.light_vel ? a.light_vel[2 * j + 1] : 0.0f;
            }
        }
    }
}

// Test entry kb_exact_selftest: the short forms of kb_exact.h with THIS chip's seeds (v_sqrt_f32, v_rsq_f32, v_rcp_f32) against
// the compiler's sqrtf(x), 1.0f / x and a / K over all 2^32 bit patterns, each form on the operands the position sweep gives it.
// counts[2 f] = operands checked, counts[2 f + 1] = results that differ in a bit; f = 0 square root, 1 reciprocal, 2 division.
__global__ void __launch_bounds__(256) kb_exact_selftest_kernel(float kbb, float kwb, unsigned long long *counts) {
    __shared__ unsigned sh[6];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0u;
    __syncthreads();
    const float ybb = 1.0f / kbb, ywb = 1.0f / kwb;
    unsigned n[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    const unsigned low = blockIdx.x * 256u + threadIdx.x;      // 2^16 blocks: the low 24 bits; the loop: the high 8
    for (unsigned k = 0; k < 256u; ++k) {
        const unsigned u = (k << 24) | low;
        const float x = __uint_as_float(u);
        if (kb_exact_guard(x)) {
            const float f = kb_sqrt_refine(x, __builtin_amdgcn_sqrtf(x), __builtin_amdgcn_rsqf(x));
            n[0]++; n[1] += __float_as_uint(f) != __float_as_uint(sqrtf(x));
        }
        if (kb_exact_len_guard(x)) {
            const float f = kb_rcp_refine(x, __builtin_amdgcn_rcpf(x));
            n[2]++; n[3] += __float_as_uint(f) != __float_as_uint(1.0f / x);
        }
        const int ex = (int)((u >> 23) & 255u) - 127;
        if ((u << 1) == 0u || (ex >= KB_EXACT_C_EXP_MIN && ex <= KB_EXACT_C_EXP_MAX)) {
            n[4] += 2u;
            n[5] += __float_as_uint(kb_div_const(x, kbb, ybb)) != __float_as_uint(x / kbb);
            n[5] += __float_as_uint(kb_div_const(x, kwb, ywb)) != __float_as_uint(x / kwb);
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) if (n[i]) atomicAdd(&sh[i], n[i]);
    __syncthreads();
    if (threadIdx.x < 6 && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

// Test entry kb_debug_lds: fills (mode 0) or inspects (mode 1) the whole LDS of the CUs, so that a test can run the other
// kernels over LDS that something else has written.  One workgroup takes all 160 KiB of a CU as dynamic LDS (no static LDS
// here: it would not fit beside them).  Mode 1 stores nothing: count[0] += words equal to `word`, count[1] += words looked at.
constexpr unsigned DEBUG_LDS_WORDS = (unsigned)LDS_CU / 4u, DEBUG_LDS_THREADS = 256u;
__global__ void __launch_bounds__(256) kb_debug_lds_kernel(int mode, unsigned word, unsigned long long *count) {
    extern __shared__ unsigned kb_debug_lds_words[];
    volatile unsigned *lds = kb_debug_lds_words;
    if (mode == 0) {
        for (unsigned i = threadIdx.x; i < DEBUG_LDS_WORDS; i += DEBUG_LDS_THREADS) lds[i] = word;
        return;
    }
    unsigned hit = 0u, seen = 0u;
    for (unsigned i = threadIdx.x; i < DEBUG_LDS_WORDS; i += DEBUG_LDS_THREADS) {
        hit += lds[i] == word;
        ++seen;
    }
    for (int o = 32; o > 0; o >>= 1) {
        hit += __shfl_down(hit, o);
        seen += __shfl_down(seen, o);
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&count[0], (unsigned long long)hit);
        atomicAdd(&count[1], (unsigned long long)seen);
    }
}

thread_local char g_err[512] = "";

float kb_clampf_host(float a, float lo, float hi) { return fmaxf(lo, fminf(a, hi)); }
// (sense_reach, the reach of a sensing stencil in cells, is in kb_sense.h: kb_coverage_kernel stops its search by it)

// kb_div_const (kb_exact.h) against a / K for one divisor of the position sweep, a = -C: every mantissa of the binade of the
// largest |C| (0.2), a stride through the mantissas of every smaller binade that |C| can reach (the form is invariant under
// scaling by a power of two while nothing leaves the normal range; the stride looks for exactly that), and both zeros.
// About 1.7e7 quotients per divisor, once per process and divisor.
bool div_form_exact(float K) {
    static std::mutex mtx;
    static std::vector<std::pair<unsigned, bool>> seen;
    unsigned kbits;
    memcpy(&kbits, &K, 4);
    std::lock_guard<std::mutex> lock(mtx);
    for (const auto &e : seen) if (e.first == kbits) return e.second;
    bool ok = K > 0.0f && std::isfinite(K);
    if (ok) {
        const float y = 1.0f / K;
        auto same = [&](float a) {
            const float f = kb_div_const(a, K, y), d = a / K;
            return memcmp(&f, &d, 4) == 0;
        };
        ok = same(0.0f) && same(-0.0f);
        for (int ex = KB_EXACT_C_EXP_MIN; ok && ex <= KB_EXACT_C_EXP_MAX; ++ex) {
            const unsigned step = ex == KB_EXACT_C_EXP_MAX ? 1u : 1021u;
            unsigned bad = 0;
            for (unsigned m = 0; m < (1u << 23); m += step) {
                const unsigned u = ((unsigned)(ex + 127) << 23) | m;
                float a;
                memcpy(&a, &u, 4);
                bad += !same(a);
            }
            ok = bad == 0;
        }
    }
    seen.emplace_back(kbits, ok);
    return ok;
}

int fail(int code, const char *fmt, const char *detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

// the status of the launch that `entry` has just made
int launched(const char *entry) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return KB_OK;
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, hipGetErrorString(err));
    return KB_EHIP;
}

// the launch a sensing entry ends in: `grid` workgroups of `block` lanes with `lds` bytes of dynamic LDS, and its status
template <typename Kernel, typename... Args>
int launch(const char *entry, Kernel kernel, unsigned grid, unsigned block, int lds, void *stream, const Args &...args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), (size_t)lds, (hipStream_t)stream, args...);
    return launched(entry);
}
// whether every one of the pointers lies on 16 bytes (NULL does)
template <typename... T>
bool aligned16(const T *...ptr) { return ((reinterpret_cast<uintptr_t>(ptr) | ...) & 15u) == 0; }
// the reach in cells of the stencil that finds everything within Rw world units (a radius beyond the arena: the stencil is the
// whole grid, and the reach stays a small integer)
int reach_cells(const Params &p, float Rw) { return Rw * p.inv_cell < (float)(p.gw + p.gh) ? sense_reach(Rw, p.inv_cell) : p.gw + p.gh; }

// a sensing radius in metres as the kernels take it: in world units, squared, and as the reach of the stencil in cells
struct SenseRange { float Rw, R2; int reach; };
SenseRange sense_range(const Params &p, float radius_m) {
    const float Rw = radius_m * WORLD_SCALE;
    return {Rw, Rw * Rw, reach_cells(p, Rw)};
}

// n_sectors of the histogram entries, reported under the caller's name
int check_sectors(const char *entry, int n_sectors) {
    if (n_sectors == 1 || (n_sectors >= 2 && n_sectors <= KB_HIST_MAX_SECTORS && !(n_sectors & 1))) return KB_OK;
    return fail(KB_EINVAL, "%s: n_sectors must be 1 or an even number in 2..KB_HIST_MAX_SECTORS (16)", entry);
}

// the instantiation of kb_reduce_kernel for an op and a channel count: rows of 1, 2, 4 or 8 words
using kb_reduce_fn = void (*)(Params, int, float, int, int, float, const float *, float *, unsigned *);
template <int OP>
kb_reduce_fn reduce_kernel(int CP) {
    return CP == 1 ? kb_reduce_kernel<OP, 1> : CP == 2 ? kb_reduce_kernel<OP, 2> : CP == 4 ? kb_reduce_kernel<OP, 4> : kb_reduce_kernel<OP, 8>;
}

// the instantiation of kb_field_kernel that holds a plane of `cells` cells: the fewest cells per lane of 4 x (1, 2, 4, 6, 8)
using kb_field_fn = void (*)(FieldArgs, const float *, const float *, const float *, const uint8_t *, const float *, float *, float4 *);
template <bool VEC>
kb_field_fn field_kernel(int cells) {
    const int per_lane = (cells + FIELD_THREADS - 1) / FIELD_THREADS;
    return per_lane <= 4 ? kb_field_kernel<1, VEC> : per_lane <= 8 ? kb_field_kernel<2, VEC> : per_lane <= 16 ? kb_field_kernel<4, VEC>
         : per_lane <= 24 ? kb_field_kernel<6, VEC> : kb_field_kernel<8, VEC>;
}

}  // namespace

struct kb_sim {
    kb_config cfg;
    Params p;
    bool bound;
    const void *attr_fn;   // kernel whose dynamic-LDS limit has been raised
    const void *paths_attr_fn;     // ... and the same for kb_sense_paths above GRID_LDS_LIMIT
    int threads;
    kb_step_fn fn;         // the instantiation that runs the handle (plan_launch), nullptr if the library has none
    int variant;           // ... and its position in kb_variants, -1 likewise (kb_variant_index)
};

kb_step_fn kb::kb_kernels[NUM_VARIANTS];

// what of a handle decides its launch shape (kb_launch.h); threads: the workgroup size asked for, 0 = choose
static PlanInput plan_input(const kb_sim *s, int threads) {
    const kb_config &c = s->cfg;
    const int nfix = c.num_fixtures > 0 ? c.num_fixtures : c.num_objects;
    bool discs = c.num_objects > 0;
    for (int f = 0; f < nfix; ++f) discs = discs && c.obj_shape[f] == KB_SHAPE_CIRCLE;
    return {c.num_bots, c.num_objects, nfix, discs, c.drive_mode, c.light_type, c.sense_radius > 0.0f, c.allow_sleep != 0,
            s->p.ncell, c.contact_capacity, threads};
}

// the launch shape into the handle (kb_create, kb_set_block_threads)
static void use_plan(kb_sim *s, const Plan &pl) {
    Params &p = s->p;
    p.cap = pl.cap; p.capL = pl.capL; p.nhead = pl.nhead; p.hmask = pl.hmask;
    p.lds_total = pl.lds_total; p.islmin_off = pl.islmin_off; p.botlaw_off = pl.botlaw_off;
    s->threads = pl.threads;
    const int i = variant_index(pl.variant);
    s->fn = i < 0 ? nullptr : kb_kernels[i];
    s->variant = s->fn ? i : -1;
}

extern "C" {

const char *kb_last_error(void) { return g_err; }
const char *kb_version(void) { return "kilobots_hip 0.1 (gfx950)"; }

int kb_create(const kb_config *cfg, kb_sim **out) {
    if (!cfg || !out) return fail(KB_EINVAL, "kb_create: NULL argument");
    if (cfg->num_envs < 1 || cfg->num_bots < 1 || cfg->num_bots > KB_MAX_BOTS)
        return fail(KB_EINVAL, "kb_create: num_envs >= 1 and 1 <= num_bots <= 1024 required");
    if (cfg->num_objects < 0 || cfg->num_objects > KB_MAX_OBJECTS) return fail(KB_EINVAL, "kb_create: 0 <= num_objects <= 8 required");
    const int nfix = cfg->num_fixtures > 0 ? cfg->num_fixtures : cfg->num_objects;
    if (cfg->num_fixtures != 0 && (cfg->num_fixtures < cfg->num_objects || cfg->num_fixtures > KB_MAX_OBJECTS))
        return fail(KB_EINVAL, "kb_create: num_fixtures must be 0 or num_objects..8");
    {
        int per_body[KB_MAX_OBJECTS] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int f = 0; f < nfix; ++f) {
            const int b = cfg->num_fixtures > 0 ? cfg->obj_fixture_body[f] : f;
            if (b < 0 || b >= cfg->num_objects) return fail(KB_EINVAL, "kb_create: obj_fixture_body out of range");
            per_body[b]++;
            if (cfg->obj_shape[f] == KB_SHAPE_CIRCLE && per_body[b] > 1) return fail(KB_EINVAL, "kb_create: a circle must be the only fixture of its object");
        }
        for (int b = 0; b < cfg->num_objects; ++b) {
            if (per_body[b] == 0) return fail(KB_EINVAL, "kb_create: every object needs a fixture");
            if (per_body[b] > 1)
                for (int f = 0; f < nfix; ++f)
                    if (cfg->obj_fixture_body[f] == b && cfg->obj_shape[f] == KB_SHAPE_CIRCLE)
                        return fail(KB_EINVAL, "kb_create: a circle must be the only fixture of its object");
        }
    }
    for (int m = 0; m < nfix; ++m) {
        const int sh = cfg->obj_shape[m];
        if (sh < KB_SHAPE_CIRCLE || sh > KB_SHAPE_POLYGON) return fail(KB_EINVAL, "kb_create: bad obj_shape");
        if (sh == KB_SHAPE_CIRCLE && !(cfg->obj_radius[m] > 0.0f)) return fail(KB_EINVAL, "kb_create: obj_radius must be positive");
        if (sh == KB_SHAPE_BOX && !(cfg->obj_verts[m][0][0] > 0.0f && cfg->obj_verts[m][0][1] > 0.0f))
            return fail(KB_EINVAL, "kb_create: box half extents (obj_verts[m][0]) must be positive");
        if (sh == KB_SHAPE_POLYGON) {
            const int n = cfg->obj_nverts[m];
            if (n < 3 || n > KB_MAX_POLY_VERTS) return fail(KB_EINVAL, "kb_create: polygons need 3..4 vertices");
            for (int i = 0; i < n; ++i) {       // counter-clockwise and convex
                const float *p0 = cfg->obj_verts[m][i], *p1 = cfg->obj_verts[m][(i + 1) % n], *p2 = cfg->obj_verts[m][(i + 2) % n];
                if (!((p1[0] - p0[0]) * (p2[1] - p1[1]) - (p1[1] - p0[1]) * (p2[0] - p1[0]) > 0.0f))
                    return fail(KB_EINVAL, "kb_create: polygon vertices must form a counter-clockwise convex hull");
            }
        }
    }
    if (cfg->num_objects > 0 && (!(cfg->obj_friction >= 0.0f) || !(cfg->wall_friction >= 0.0f)))
        return fail(KB_EINVAL, "kb_create: friction coefficients must be non-negative");
    if (cfg->num_objects > 0 && !(cfg->obj_density > 0.0f)) return fail(KB_EINVAL, "kb_create: obj_density must be positive");
    if (cfg->drive_mode < 0 || cfg->drive_mode > KB_DRIVE_MIXED) return fail(KB_EINVAL, "kb_create: bad drive_mode");
    if (cfg->light_type < KB_LIGHT_NONE || cfg->light_type > KB_LIGHT_COMPOSITE)
        return fail(KB_EINVAL, "kb_create: unsupported light_type");
    if (cfg->light_type == KB_LIGHT_COMPOSITE) {
        if (cfg->light_count < 1 || cfg->light_count > KB_MAX_LIGHTS) return fail(KB_EINVAL, "kb_create: 1 <= light_count <= 4 required");
        for (int i = 0; i < cfg->light_count; ++i)
            if (cfg->light_kind[i] != KB_LIGHT_CIRCULAR && cfg->light_kind[i] != KB_LIGHT_MOMENTUM)
                return fail(KB_EINVAL, "kb_create: composite components must be circular or momentum lights");
    }
    if ((cfg->drive_mode == KB_DRIVE_SIMPLE_PHOTOTAXIS || cfg->drive_mode == KB_DRIVE_PHOTOTAXIS) &&
        cfg->light_type == KB_LIGHT_NONE)
        return fail(KB_EINVAL, "kb_create: phototaxis drive modes need a light");
    if (cfg->ws_slots < 1 || cfg->ws_slots > 64) return fail(KB_EINVAL, "kb_create: 1 <= ws_slots <= 64 required");
    if (cfg->solver_mode < 0 || cfg->solver_mode > 4) return fail(KB_EINVAL, "kb_create: solver_mode must be 0..4");
    if (cfg->damping_model != KB_DAMPING_PADE && cfg->damping_model != KB_DAMPING_LINEAR) return fail(KB_EINVAL, "kb_create: damping_model must be KB_DAMPING_PADE or KB_DAMPING_LINEAR");
    if (!(cfg->sense_radius >= 0.0f)) return fail(KB_EINVAL, "kb_create: sense_radius must be >= 0");
    if (cfg->contact_capacity < 0 || cfg->contact_capacity > 65528) return fail(KB_EINVAL, "kb_create: 0 <= contact_capacity <= 65528 required");
    if (!(cfg->dt > 0.0f) || cfg->vel_iters < 0 || cfg->pos_iters < 0 || !(cfg->world_width > 0.0f) ||
        !(cfg->world_height > 0.0f) || !(cfg->bot_radius > 0.0f) || !(cfg->bot_density > 0.0f))
        return fail(KB_EINVAL, "kb_create: non-positive dt / size / radius / density");
    kb_sim *s = new (std::nothrow) kb_sim();
    if (!s) return fail(KB_EINVAL, "kb_create: out of host memory");
    s->cfg = *cfg;
    s->bound = false;
    s->attr_fn = nullptr;
    s->paths_attr_fn = nullptr;
    Params &p = s->p;
    memset(&p, 0, sizeof(p));
    p.N = cfg->num_bots; p.E = cfg->num_envs; p.S = cfg->ws_slots;
    p.allow_sleep = cfg->allow_sleep != 0;
    p.drive_mode = cfg->drive_mode; p.light_type = cfg->light_type;
    p.vel_iters = cfg->vel_iters; p.pos_iters = cfg->pos_iters;
    const float W = cfg->world_width * WORLD_SCALE, H = cfg->world_height * WORLD_SCALE;
    p.xmin = -0.5f * W; p.xmax = 0.5f * W; p.ymin = -0.5f * H; p.ymax = 0.5f * H;
    float cell = CELL_SIZE;
    const float dmin = 2.0f * cfg->bot_radius * WORLD_SCALE;
    while (cell < dmin) cell *= 2.0f;
    for (;;) {
        p.inv_cell = 1.0f / cell;
        p.gw = (int)ceilf(W * p.inv_cell); if (p.gw < 1) p.gw = 1;
        p.gh = (int)ceilf(H * p.inv_cell); if (p.gh < 1) p.gh = 1;
        if ((long)p.gw * p.gh <= MAX_CELLS) break;
        cell *= 2.0f;
    }
    p.ncell = p.gw * p.gh;
    p.h = cfg->dt;
    p.r_bot = cfg->bot_radius * WORLD_SCALE;
    const float m = cfg->bot_density * B2_PI * p.r_bot * p.r_bot;  // b2CircleShape::ComputeMass
    p.im_bot = m > 0.0f ? 1.0f / m : 0.0f;
    {
        const float rr = p.r_bot + p.r_bot, rw = B2_POLYGON_RADIUS + p.r_bot;
        p.rr2 = rr * rr; p.rw2 = rw * rw; p.rw_tot = p.r_bot + B2_POLYGON_RADIUS;
        p.toi_tt = fmaxf(B2_LINEAR_SLOP, p.rw_tot - 3.0f * B2_LINEAR_SLOP) + 0.25f * B2_LINEAR_SLOP;      // kb_toi_wall: target + tol
        const float kbb = p.im_bot + p.im_bot, kwb = 0.0f + p.im_bot;
        p.nm_bb = kbb > 0.0f ? 1.0f / kbb : 0.0f; p.nm_wb = kwb > 0.0f ? 1.0f / kwb : 0.0f;
        // the position sweep divides -C by these two: by multiplying, if the short form gives the quotient's bits for them
        p.exact_div = div_form_exact(kbb) && div_form_exact(kwb);
        p.y_bb = p.exact_div ? 1.0f / kbb : 0.0f; p.y_wb = p.exact_div ? 1.0f / kwb : 0.0f;
    }
    for (int k = 0; k < 5; ++k) {       // KB_DRIVE_MIXED: the classes have different fixture densities (kilobot.py:25 / :214)
        p.im_mode[k] = p.im_bot;
        if (cfg->drive_mode == KB_DRIVE_MIXED && cfg->mode_density[k] > 0.0f) {
            const float mk = cfg->mode_density[k] * B2_PI * p.r_bot * p.r_bot;
            p.im_mode[k] = mk > 0.0f ? 1.0f / mk : 0.0f;
        }
    }
    // b2Island::Solve damping factor per step: Pade (Box2D >= 2.3.1) or the older clamped linear form
    auto damp = [&](float c) -> float {
        if (cfg->damping_model == KB_DAMPING_LINEAR) return kb_clampf_host(1.0f - p.h * c, 0.0f, 1.0f);
        return 1.0f / (1.0f + p.h * c);
    };
    p.kl_bot = damp(cfg->bot_linear_damping);
    p.ka_bot = damp(cfg->bot_angular_damping);
    p.light_radius = cfg->light_radius;
    p.lcount = cfg->light_type == KB_LIGHT_COMPOSITE ? cfg->light_count : 1;
    p.ladim = cfg->light_type == KB_LIGHT_NONE ? 0 : (cfg->light_type == KB_LIGHT_GRADIENT ? 1 : 2 * p.lcount);
    for (int i = 0; i < KB_MAX_LIGHTS; ++i) {
        const bool comp = cfg->light_type == KB_LIGHT_COMPOSITE;
        p.lkind[i] = comp ? cfg->light_kind[i] : cfg->light_type;
        p.lradius[i] = comp ? cfg->lightc_radius[i] : cfg->light_radius;
        p.lmaxv[i] = comp ? cfg->lightc_max_velocity[i] : cfg->light_max_velocity;
        for (int k = 0; k < 2; ++k) {
            p.llo[i][k] = comp ? cfg->lightc_lo[i][k] : cfg->light_lo[k];
            p.lhi[i][k] = comp ? cfg->lightc_hi[i][k] : cfg->light_hi[k];
            p.lalo[i][k] = comp ? cfg->lightc_act_lo[i][k] : cfg->light_act_lo[k];
            p.lahi[i][k] = comp ? cfg->lightc_act_hi[i][k] : cfg->light_act_hi[k];
        }
    }
    for (int i = 0; i < 2; ++i) {
        p.light_lo[i] = cfg->light_lo[i]; p.light_hi[i] = cfg->light_hi[i];
        p.act_lo[i] = cfg->light_act_lo[i]; p.act_hi[i] = cfg->light_act_hi[i];
    }
    p.NP = (p.N + 3) & ~3;
    p.NB = p.NP + KB_MAX_OBJECTS + 4;
    p.M = cfg->num_objects;
    p.F = nfix;
    float bm[KB_MAX_OBJECTS], bi[KB_MAX_OBJECTS];
    V2 bc[KB_MAX_OBJECTS];
    for (int m = 0; m < KB_MAX_OBJECTS; ++m) { bm[m] = 0.0f; bi[m] = 0.0f; bc[m] = mk2(0.0f, 0.0f); }
    for (int f = 0; f < KB_MAX_OBJECTS; ++f) {
        float *T = p.otab[f];
        for (int k = 0; k < OT_WORDS; ++k) T[k] = 0.0f;
        if (f >= nfix) continue;
        const int body = cfg->num_fixtures > 0 ? cfg->obj_fixture_body[f] : f;
        const int kind = cfg->obj_shape[f];
        float mo, io;
        V2 ce = mk2(0.0f, 0.0f);
        T[OT_KIND] = (float)kind; T[OT_N] = 0.0f; T[OT_BODY] = (float)body;
        if (kind == KB_SHAPE_CIRCLE) {
            const float r = cfg->obj_radius[f] * WORLD_SCALE;
            T[OT_RADIUS] = r;
            mo = cfg->obj_density * B2_PI * r * r;       // b2CircleShape::ComputeMass
            io = mo * (0.5f * r * r);                     // I = mass * (0.5 r^2 + |p|^2), p = 0
        } else {
            int n;
            if (kind == KB_SHAPE_BOX) {                   // b2PolygonShape::SetAsBox
                const float hx = cfg->obj_verts[f][0][0], hy = cfg->obj_verts[f][0][1];
                n = 4;
                const float vx[4] = {-hx, hx, hx, -hx}, vy[4] = {-hy, -hy, hy, hy};
                const float nx[4] = {0.0f, 1.0f, 0.0f, -1.0f}, ny[4] = {-1.0f, 0.0f, 1.0f, 0.0f};
                for (int i = 0; i < 4; ++i) {
                    T[OT_VERTS + 2 * i] = vx[i]; T[OT_VERTS + 2 * i + 1] = vy[i];
                    T[OT_NORMALS + 2 * i] = nx[i]; T[OT_NORMALS + 2 * i + 1] = ny[i];
                }
            } else {                                      // b2PolygonShape::Set on an ordered hull
                n = cfg->obj_nverts[f];
                for (int i = 0; i < n; ++i) {
                    T[OT_VERTS + 2 * i] = cfg->obj_verts[f][i][0];
                    T[OT_VERTS + 2 * i + 1] = cfg->obj_verts[f][i][1];
                }
                for (int i = 0; i < n; ++i) {
                    const V2 edge = v_sub(ot_v(T, i + 1 < n ? i + 1 : 0), ot_v(T, i));
                    const V2 nr = v_normalize(v_cross_vs(edge, 1.0f));
                    T[OT_NORMALS + 2 * i] = nr.x; T[OT_NORMALS + 2 * i + 1] = nr.y;
                }
            }
            T[OT_N] = (float)n;
            T[OT_RADIUS] = B2_POLYGON_RADIUS;
            polygon_mass(T, cfg->obj_density, mo, ce, io);
        }
        bm[body] += mo; bc[body] = v_add(bc[body], v_scale(mo, ce)); bi[body] += io;      // b2Body::ResetMassData
    }
    for (int m = 0; m < KB_MAX_OBJECTS; ++m) {
        float *B = p.obody[m];
        for (int k = 0; k < BT_WORDS; ++k) B[k] = 0.0f;
        V2 lc = mk2(0.0f, 0.0f);
        if (bm[m] > 0.0f) { B[BT_IM] = 1.0f / bm[m]; lc = v_scale(B[BT_IM], bc[m]); }
        const float io = bi[m] - bm[m] * v_dot(lc, lc);     // inertia about the centre of mass
        B[BT_II] = io > 0.0f ? 1.0f / io : 0.0f;
        B[BT_LCX] = lc.x; B[BT_LCY] = lc.y;
        B[BT_RADIUS] = B2_POLYGON_RADIUS;
    }
    for (int f = 0; f < nfix; ++f) {
        float *T = p.otab[f];
        const int body = ot_body(T);
        float *B = p.obody[body];
        T[OT_IM] = B[BT_IM]; T[OT_II] = B[BT_II];
        B[BT_KIND] = T[OT_KIND];
        if (ot_kind(T) == KB_SHAPE_CIRCLE) { T[OT_BOUND] = T[OT_RADIUS]; B[BT_RADIUS] = T[OT_RADIUS]; continue; }
        float far2 = 0.0f;                                // bounding radius about the centre of mass of the body
        for (int i = 0; i < ot_n(T); ++i) { const V2 q = v_sub(ot_v(T, i), mk2(B[BT_LCX], B[BT_LCY])); far2 = fmaxf(far2, v_dot(q, q)); }
        T[OT_BOUND] = sqrtf(far2) + B2_POLYGON_RADIUS;
    }
    p.mu_oo = sqrtf(cfg->obj_friction * cfg->obj_friction);
    p.mu_ow = sqrtf(cfg->obj_friction * cfg->wall_friction);
    p.nmc = mc_candidates(p.F);
    p.kl_obj = damp(cfg->obj_linear_damping);
    p.ka_obj = damp(cfg->obj_angular_damping);
    p.sense_s = 0; p.sense_r2 = 0.0f;
    if (cfg->sense_radius > 0.0f) {
        const float Rw = cfg->sense_radius * WORLD_SCALE;
        p.sense_s = sense_reach(Rw, p.inv_cell);
        p.sense_r2 = Rw * Rw;
    }
    p.solver_mode = cfg->solver_mode;
    p.toi_walls = cfg->toi_walls;
    const Plan pl = plan_launch(plan_input(s, 0));
    if (pl.status != KB_OK) { delete s; return fail(pl.status, "%s", pl.msg); }
    use_plan(s, pl);
    *out = s;
    return KB_OK;
}

void kb_destroy(kb_sim *sim) { delete sim; }

int kb_bind(kb_sim *sim, const kb_buffers *b) {
    if (!sim || !b) return fail(KB_EINVAL, "kb_bind: NULL argument");
    if (!b->x || !b->y || !b->theta || !b->ws_key || !b->ws_acc || !b->ws_cnt || !b->status || !b->scratch)
        return fail(KB_ENOTBOUND, "kb_bind: x, y, theta, ws_key, ws_acc, ws_cnt, status and scratch are required");
    const int m = sim->cfg.drive_mode;
    if (m == KB_DRIVE_MIXED && (!b->bot_mode || !b->v || !b->w || !b->acc_v || !b->acc_w || !b->motor_l || !b->motor_r ||
                                !b->pt_threshold || !b->pt_update || !b->pt_nochange || !b->pt_dir))
        return fail(KB_ENOTBOUND, "kb_bind: KB_DRIVE_MIXED needs bot_mode and the state buffers of every drive law");
    if ((m == KB_DRIVE_VELOCITY || m == KB_DRIVE_ACCEL) && (!b->v || !b->w))
        return fail(KB_ENOTBOUND, "kb_bind: v and w are required in the velocity / acceleration modes");
    if (m == KB_DRIVE_ACCEL && (!b->acc_v || !b->acc_w)) return fail(KB_ENOTBOUND, "kb_bind: acc_v, acc_w required");
    if ((m == KB_DRIVE_MOTORS || m == KB_DRIVE_PHOTOTAXIS) && (!b->motor_l || !b->motor_r))
        return fail(KB_ENOTBOUND, "kb_bind: motor_l, motor_r required");
    if (m == KB_DRIVE_PHOTOTAXIS && (!b->pt_threshold || !b->pt_update || !b->pt_nochange || !b->pt_dir))
        return fail(KB_ENOTBOUND, "kb_bind: pt_* buffers required in the phototaxis mode");
    if (sim->cfg.num_objects > 0 && (!b->ox || !b->oy || !b->otheta || !b->ovx || !b->ovy || !b->ow || !b->ows_acc))
        return fail(KB_ENOTBOUND, "kb_bind: ox, oy, otheta, ovx, ovy, ow and ows_acc are required when num_objects > 0");
    if (sim->cfg.light_type != KB_LIGHT_NONE && (!b->light_x || (!b->light_y && sim->cfg.light_type != KB_LIGHT_GRADIENT)))
        return fail(KB_ENOTBOUND, "kb_bind: light_x, light_y required when a light is configured");
    {
        bool momentum = sim->cfg.light_type == KB_LIGHT_MOMENTUM;
        if (sim->cfg.light_type == KB_LIGHT_COMPOSITE)
            for (int i = 0; i < sim->cfg.light_count; ++i) momentum |= sim->cfg.light_kind[i] == KB_LIGHT_MOMENTUM;
        if (momentum && (!b->light_vx || !b->light_vy)) return fail(KB_ENOTBOUND, "kb_bind: light_vx, light_vy required by a MomentumLight");
    }
    if ((b->light_value != nullptr) != (b->light_gx != nullptr) || (b->light_value != nullptr) != (b->light_gy != nullptr))
        return fail(KB_EINVAL, "kb_bind: light_value, light_gx, light_gy must be given together");
    if ((b->cmd_vx != nullptr) != (b->cmd_vy != nullptr) || (b->cmd_vx != nullptr) != (b->cmd_w != nullptr))
        return fail(KB_EINVAL, "kb_bind: cmd_vx, cmd_vy, cmd_w must be given together");
    if (sim->cfg.sense_radius > 0.0f && !b->nbr_count) return fail(KB_ENOTBOUND, "kb_bind: nbr_count is required when sense_radius > 0");
    if (sim->cfg.allow_sleep && (!b->sleep_time || (sim->cfg.num_objects > 0 && !b->osleep)))
        return fail(KB_ENOTBOUND, "kb_bind: sleep_time (and osleep with objects) are required when allow_sleep is set");
    sim->p.buf = *b;
    sim->bound = true;
    return KB_OK;
}

int kb_set_actions(kb_sim *sim, const float *d_actions, void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_set_actions: NULL handle");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_set_actions: kb_bind() first");
    if (sim->cfg.drive_mode != KB_DRIVE_VELOCITY && sim->cfg.drive_mode != KB_DRIVE_ACCEL && sim->cfg.drive_mode != KB_DRIVE_MIXED)
        return fail(KB_EINVAL, "kb_set_actions: only the velocity / acceleration drive modes take actions");
    Params p = sim->p;
    p.actions = d_actions;
    const size_t T = (size_t)p.E * p.N;
    hipLaunchKernelGGL(kb_set_actions_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launched("kb_set_actions");
}

int kb_resident_envs_per_cu(kb_sim *sim) {
    if (!sim) return fail(KB_EINVAL, "kb_resident_envs_per_cu: NULL handle");
    const kb_step_fn fn = sim->fn;
    if (!fn) return fail(KB_EINVAL, "kb_resident_envs_per_cu: no kernel for this configuration");
    if (sim->p.lds_total > 64 * 1024) {
        hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CU);
        if (e2 != hipSuccess) return fail(KB_EHIP, "kb_resident_envs_per_cu: hipFuncSetAttribute: %s", hipGetErrorString(e2));
    }
    int n = 0;
    hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(fn), sim->threads, (size_t)sim->p.lds_total);
    if (err != hipSuccess) return fail(KB_EHIP, "kb_resident_envs_per_cu: %s", hipGetErrorString(err));
    return n;
}

// the one launch of kb_step and kb_step_envs (d_env_mask NULL: every env), reported under the caller's name
static int step_launch(const char *entry, kb_sim *sim, const uint8_t *d_env_mask, const float *d_actions, const float *d_light_action,
                       int n_substeps, int flags, void *stream) {
    if (!sim->bound) return fail(KB_ENOTBOUND, "%s: kb_bind() first", entry);
    if (n_substeps < 0) return fail(KB_EINVAL, "%s: n_substeps < 0", entry);
    if (d_actions && sim->cfg.drive_mode != KB_DRIVE_VELOCITY && sim->cfg.drive_mode != KB_DRIVE_ACCEL && sim->cfg.drive_mode != KB_DRIVE_MIXED)
        return fail(KB_EINVAL, "%s: only the velocity / acceleration drive modes take actions", entry);
    if (n_substeps == 0 && !d_actions) return KB_OK;
    Params p = sim->p;
    p.actions = d_actions;
    p.light_action = d_light_action;
    p.env_mask = d_env_mask;
    p.n_substeps = n_substeps;
    p.flags = flags;
    const kb_step_fn fn = sim->fn;
    if (!fn) return fail(KB_EINVAL, "%s: no kernel for this drive mode / light type", entry);
    if (p.lds_total > 64 * 1024 && sim->attr_fn != reinterpret_cast<const void *>(fn)) {
        // the attribute belongs to the kernel, not to this sim: raise it to the hardware limit, so that sims of
        // different sizes sharing one instantiation never lower it under each other
        hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void *>(fn),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CU);
        if (e2 != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: hipFuncSetAttribute: %s", entry, hipGetErrorString(e2)); return KB_EHIP; }
        sim->attr_fn = reinterpret_cast<const void *>(fn);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)p.E), dim3((unsigned)sim->threads), (size_t)p.lds_total,
                       (hipStream_t)stream, p);
    return launched(entry);
}

int kb_step(kb_sim *sim, const float *d_actions, const float *d_light_action, int n_substeps, int flags, void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_step: NULL handle");
    return step_launch("kb_step", sim, nullptr, d_actions, d_light_action, n_substeps, flags, stream);
}

int kb_step_envs(kb_sim *sim, const uint8_t *d_env_mask, const float *d_actions, const float *d_light_action, int n_substeps, int flags,
                 void *stream) {
    if (!sim || !d_env_mask) return fail(KB_EINVAL, "kb_step_envs: NULL argument");
    return step_launch("kb_step_envs", sim, d_env_mask, d_actions, d_light_action, n_substeps, flags, stream);
}

int kb_sense(kb_sim *sim, float radius_m, uint32_t *d_count, void *stream) {
    if (!sim || !d_count) return fail(KB_EINVAL, "kb_sense: NULL argument");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense: kb_bind() first");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense: radius must be positive");
    const Params &p = sim->p;
    const SenseRange r = sense_range(p, radius_m);
    return launch("kb_sense", kb_sense_kernel, p.E, 256, SenseLds(p.NP, p.ncell).bytes, stream, p, r.reach, r.R2, d_count);
}

int kb_sense_neighbors(kb_sim *sim, float radius_m, int k, int32_t *d_index, float *d_rel, uint32_t *d_count, void *stream) {
    if (!sim || !d_index || !d_rel) return fail(KB_EINVAL, "kb_sense_neighbors: NULL argument");
    if (k < 1 || k > KB_MAX_NEIGHBORS) return fail(KB_EINVAL, "kb_sense_neighbors: 1 <= k <= KB_MAX_NEIGHBORS (16) required");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_neighbors: radius must be positive");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_neighbors: kb_bind() first");
    if (!aligned16(d_rel)) return fail(KB_EINVAL, "kb_sense_neighbors: d_rel must be 16-byte aligned");
    const Params &p = sim->p;
    const SenseRange r = sense_range(p, radius_m);
    const int vec = k % 4 == 0 && aligned16(d_index);
    const auto fn = k <= 4 ? kb_neighbors_kernel<4> : k <= 8 ? kb_neighbors_kernel<8> : kb_neighbors_kernel<16>;
    return launch("kb_sense_neighbors", fn, p.E, 256, NeighborsLds(p.NP, p.ncell).bytes, stream, p, r.reach, r.R2, k, vec, d_index, reinterpret_cast<float4 *>(d_rel), d_count);
}

int kb_sense_edges(kb_sim *sim, float radius_m, const int64_t *d_offsets, int64_t capacity, int32_t *d_src, int32_t *d_dst, float *d_rel,
                   uint32_t *d_count, void *stream) {
    if (!sim || !d_offsets) return fail(KB_EINVAL, "kb_sense_edges: NULL argument");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_edges: radius must be positive");
    if (capacity < 0) return fail(KB_EINVAL, "kb_sense_edges: capacity must not be negative");
    if (capacity > 0 && !d_dst) return fail(KB_EINVAL, "kb_sense_edges: NULL d_dst with a capacity");
    const Params &p = sim->p;
    // (a property of the handle: refused before anything is asked of its buffers, which at this size nobody can bind)
    if ((long long)p.E * p.N >= (1ll << 31)) return fail(KB_EINVAL, "kb_sense_edges: num_envs * num_bots must be below 2^31 (int32 node ids)");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_edges: kb_bind() first");
    if (!aligned16(d_rel)) return fail(KB_EINVAL, "kb_sense_edges: d_rel must be 16-byte aligned");
    if (capacity == 0 && !d_count) return KB_OK;        // nothing to write: nothing is launched
    const SenseRange r = sense_range(p, radius_m);
    return launch("kb_sense_edges", kb_edges_kernel, p.E, 256, EdgesLds(p.N, p.NP, p.ncell).bytes, stream, p, r.reach, r.R2,
                  reinterpret_cast<const long long *>(d_offsets), (long long)capacity, d_src, d_dst, reinterpret_cast<float4 *>(d_rel), d_count);
}

int kb_histogram_sectors(int n_sectors, float *xy) {
    if (check_sectors("kb_histogram_sectors", n_sectors) != KB_OK) return KB_EINVAL;
    const int H = n_sectors / 2;
    if (H > 1 && !xy) return fail(KB_EINVAL, "kb_histogram_sectors: NULL table");
    for (int m = 1; m < H; ++m) {
        const double t = 3.14159265358979323846 * (double)m / (double)H;
        xy[2 * (m - 1) + 0] = 2 * m == H ? 0.0f : (float)cos(t);
        xy[2 * (m - 1) + 1] = 2 * m == H ? 1.0f : (float)sin(t);
    }
    return KB_OK;
}

int kb_sense_histogram(kb_sim *sim, float radius_m, int n_rings, int n_sectors, float *d_hist, uint32_t *d_count, void *stream) {
    if (!sim || !d_hist) return fail(KB_EINVAL, "kb_sense_histogram: NULL argument");
    if (n_rings < 1 || n_rings > KB_HIST_MAX_RINGS) return fail(KB_EINVAL, "kb_sense_histogram: 1 <= n_rings <= KB_HIST_MAX_RINGS (8) required");
    if (check_sectors("kb_sense_histogram", n_sectors) != KB_OK) return KB_EINVAL;
    if (n_rings * n_sectors > KB_HIST_MAX_BINS) return fail(KB_EINVAL, "kb_sense_histogram: n_rings * n_sectors <= KB_HIST_MAX_BINS (64) required");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_histogram: radius must be positive");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_histogram: kb_bind() first");
    const Params &p = sim->p;
    const SenseRange rg = sense_range(p, radius_m);
    HistArgs h;
    memset(&h, 0, sizeof(h));
    h.n_rings = n_rings; h.n_sectors = n_sectors;
    // the kernel's comparisons are branch-free over the whole tables: an edge at infinity and a zero boundary vector count nothing
    for (int r = 1; r < KB_HIST_MAX_RINGS; ++r) {
        const float edge = (rg.Rw * (float)r) / (float)n_rings;
        h.e2[r - 1] = r < n_rings ? edge * edge : INFINITY;
    }
    float u[KB_HIST_MAX_SECTORS / 2 - 1][2];
    if (kb_histogram_sectors(n_sectors, &u[0][0]) != KB_OK) return KB_EINVAL;
    for (int m = 1; m < n_sectors / 2; ++m) { h.ux[m - 1] = u[m - 1][0]; h.uy[m - 1] = u[m - 1][1]; }
    return launch("kb_sense_histogram", kb_histogram_kernel, p.E, 256, HistLds(p.NP, p.ncell, n_rings * n_sectors).bytes, stream, p, rg.reach, rg.R2, h, d_hist, d_count);
}

int kb_sense_reduce(kb_sim *sim, float radius_m, int op, int n_channels, float scale, const float *d_values, float *d_out,
                    uint32_t *d_count, void *stream) {
    if (!sim || !d_values || !d_out) return fail(KB_EINVAL, "kb_sense_reduce: NULL argument");
    if (op != KB_REDUCE_SUM && op != KB_REDUCE_MIN && op != KB_REDUCE_MAX) return fail(KB_EINVAL, "kb_sense_reduce: op must be KB_REDUCE_SUM, KB_REDUCE_MIN or KB_REDUCE_MAX");
    if (n_channels < 1 || n_channels > KB_REDUCE_MAX_CHANNELS) return fail(KB_EINVAL, "kb_sense_reduce: 1 <= n_channels <= KB_REDUCE_MAX_CHANNELS (8) required");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_reduce: radius must be positive");
    if (op == KB_REDUCE_SUM && !(scale > 0.0f && scale < INFINITY)) return fail(KB_EINVAL, "kb_sense_reduce: scale must be finite and positive");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_reduce: kb_bind() first");
    const Params &p = sim->p;
    const SenseRange r = sense_range(p, radius_m);
    const int CP = n_channels <= 2 ? n_channels : n_channels <= 4 ? 4 : 8;
    const int vec = n_channels % 4 == 0 && aligned16(d_out);
    const kb_reduce_fn fn = op == KB_REDUCE_SUM ? reduce_kernel<KB_REDUCE_SUM>(CP) : op == KB_REDUCE_MIN ? reduce_kernel<KB_REDUCE_MIN>(CP) : reduce_kernel<KB_REDUCE_MAX>(CP);
    return launch("kb_sense_reduce", fn, p.E, 256, ReduceLds(p.NP, p.ncell, CP).bytes, stream, p, r.reach, r.R2, n_channels, vec, scale, d_values, d_out, d_count);
}

int kb_sense_hops(kb_sim *sim, float radius_m, const uint8_t *d_seed, int max_hops, int32_t *d_hops, int32_t *d_parent, int32_t *d_root,
                  int32_t *d_stats, void *stream) {
    if (!sim || !d_seed || !d_hops) return fail(KB_EINVAL, "kb_sense_hops: NULL argument");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_hops: radius must be positive");
    if (max_hops < 0) return fail(KB_EINVAL, "kb_sense_hops: max_hops must not be negative");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_hops: kb_bind() first");
    const Params &p = sim->p;
    const SenseRange r = sense_range(p, radius_m);
    const int lim = max_hops < p.N - 1 ? max_hops : p.N - 1;       // no path has more than N - 1 edges: the level loop's bound
    return launch("kb_sense_hops", kb_hops_kernel, p.E, 256, HopsLds(p.NP, p.ncell).bytes, stream, p, r.reach, r.R2, lim, d_seed, d_hops, d_parent, d_root, d_stats);
}

int kb_sense_clusters(kb_sim *sim, float radius_m, const uint8_t *d_select, int32_t *d_label, int32_t *d_size, float *d_cluster, int32_t *d_stats,
                      void *stream) {
    if (!sim || !d_label) return fail(KB_EINVAL, "kb_sense_clusters: NULL argument");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_clusters: radius must be positive");
    if (!aligned16(d_cluster)) return fail(KB_EINVAL, "kb_sense_clusters: d_cluster must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_clusters: kb_bind() first");
    const Params &p = sim->p;
    const SenseRange r = sense_range(p, radius_m);
    return launch("kb_sense_clusters", kb_clusters_kernel, p.E, 256, ClustersLds(p.NP, p.ncell).bytes, stream, p, r.reach, r.R2, d_select, d_label, d_size,
                  reinterpret_cast<float4 *>(d_cluster), d_stats);
}

int kb_ray_directions(int n_rays, float *xy) {
    if (n_rays < 1 || n_rays > KB_MAX_RAYS) return fail(KB_EINVAL, "kb_ray_directions: 1 <= n_rays <= KB_MAX_RAYS (32) required");
    if (!xy) return fail(KB_EINVAL, "kb_ray_directions: NULL table");
    static const float quarter[4][2] = {{1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}, {0.0f, -1.0f}};
    for (int k = 0; k < n_rays; ++k) {
        const double t = 2.0 * 3.14159265358979323846 * (double)k / (double)n_rays;
        const bool whole = (4 * k) % n_rays == 0;       // a whole number of quarter turns
        xy[2 * k + 0] = whole ? quarter[4 * k / n_rays][0] : (float)cos(t);
        xy[2 * k + 1] = whole ? quarter[4 * k / n_rays][1] : (float)sin(t);
    }
    return KB_OK;
}

int kb_sense_rays(kb_sim *sim, float radius_m, int n_rays, int targets, float *d_dist, int32_t *d_hit, void *stream) {
    if (!sim || !d_dist) return fail(KB_EINVAL, "kb_sense_rays: NULL argument");
    if (targets <= 0 || (targets & ~(KB_RAY_BOTS | KB_RAY_OBJECTS | KB_RAY_WALLS)))
        return fail(KB_EINVAL, "kb_sense_rays: targets must be a non-empty subset of KB_RAY_BOTS | KB_RAY_OBJECTS | KB_RAY_WALLS");
    if (n_rays < 1 || n_rays > KB_MAX_RAYS) return fail(KB_EINVAL, "kb_sense_rays: 1 <= n_rays <= KB_MAX_RAYS (32) required");
    if (!(radius_m > 0.0f)) return fail(KB_EINVAL, "kb_sense_rays: radius must be positive");
    if ((targets & KB_RAY_OBJECTS) && sim->cfg.num_objects == 0) return fail(KB_EINVAL, "kb_sense_rays: KB_RAY_OBJECTS asked for, but the handle has no objects");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_rays: kb_bind() first");
    const Params &p = sim->p;
    RayArgs a;
    memset(&a, 0, sizeof(a));
    a.n_rays = n_rays; a.targets = targets;
    a.Rw = radius_m * WORLD_SCALE;
    a.rb2 = p.r_bot * p.r_bot;
    const float Rc = a.Rw + p.r_bot;
    a.Rc2 = Rc * Rc;
    float u[KB_MAX_RAYS][2];
    if (kb_ray_directions(n_rays, &u[0][0]) != KB_OK) return KB_EINVAL;
    for (int k = 0; k < n_rays; ++k) { a.ux[k] = u[k][0]; a.uy[k] = u[k][1]; }
    kb_outline ol;
    kb_get_outline(sim, &ol);
    const int vec = n_rays % 4 == 0 && aligned16(d_dist, d_hit);
    // the rays a lane holds at a time: the count rounded up to 4, 8 or 16; more than that go in passes (17 to 32 rays: two of 16)
    const auto fn = n_rays <= 4 ? kb_rays_kernel<4> : n_rays <= 8 ? kb_rays_kernel<8> : kb_rays_kernel<KB_RAYS_PER_PASS>;
    return launch("kb_sense_rays", fn, p.E, 256, RaysLds(p.NP, p.ncell).bytes, stream, p, ol, a, reach_cells(p, Rc), vec, d_dist, d_hit);
}

int kb_get_outline(const kb_sim *sim, kb_outline *out) {
    if (!sim || !out) return fail(KB_EINVAL, "kb_get_outline: NULL argument");
    const Params &p = sim->p;
    memset(out, 0, sizeof(*out));
    out->num_objects = p.M;
    out->arena[0] = p.xmin; out->arena[1] = p.xmax; out->arena[2] = p.ymin; out->arena[3] = p.ymax;
    int g = 0;
    for (int b = 0; b < p.M; ++b) {             // grouped by body; within a body the kb_config order
        for (int f = 0; f < p.F; ++f) {
            const float *T = p.otab[f];
            if (ot_body(T) != b) continue;
            const bool circle = ot_kind(T) == KB_SHAPE_CIRCLE;
            out->body[g] = b; out->kind[g] = ot_kind(T); out->nverts[g] = circle ? 0 : ot_n(T);
            out->radius[g] = circle ? T[OT_RADIUS] : 0.0f;
            for (int i = 0; i < out->nverts[g]; ++i) { out->verts[g][i][0] = T[OT_VERTS + 2 * i]; out->verts[g][i][1] = T[OT_VERTS + 2 * i + 1]; }
            ++g;
        }
    }
    out->num_fixtures = g;
    return KB_OK;
}

int kb_sense_objects(kb_sim *sim, float *d_obj, float *d_wall, void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_sense_objects: NULL handle");
    if (!d_obj && !d_wall) return fail(KB_EINVAL, "kb_sense_objects: d_obj and d_wall are both NULL");
    if (d_obj && sim->cfg.num_objects == 0) return fail(KB_EINVAL, "kb_sense_objects: d_obj given, but the handle has no objects");
    if (!aligned16(d_obj, d_wall)) return fail(KB_EINVAL, "kb_sense_objects: d_obj and d_wall must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_objects: kb_bind() first");
    const Params &p = sim->p;
    kb_outline ol;
    kb_get_outline(sim, &ol);
    const int threads = p.N < OBJ_TILE ? (p.N + 63) & ~63 : OBJ_TILE;      // one kilobot per lane: no idle waves in a small env
    const int tiles = (p.N + threads - 1) / threads;
    return launch("kb_sense_objects", kb_objects_kernel, (unsigned)p.E * (unsigned)tiles, threads, ObjectsLds().bytes, stream, ol, p.N, tiles, p.buf.x, p.buf.y,
                  p.buf.theta, p.buf.ox, p.buf.oy, p.buf.otheta, reinterpret_cast<float4 *>(d_obj), reinterpret_cast<float4 *>(d_wall));
}

// planes of the grid entries, reported under the caller's name: a non-empty subset of the three bits ...
static int check_grid_planes(const char *entry, int planes) {
    if (planes > 0 && !(planes & ~(KB_GRID_COUNT | KB_GRID_FLOW | KB_GRID_OBJECTS))) return KB_OK;
    return fail(KB_EINVAL, "%s: planes must be a non-empty subset of KB_GRID_COUNT | KB_GRID_FLOW | KB_GRID_OBJECTS", entry);
}
// ... and the objects only of a handle that has some
static int check_grid_objects(const char *entry, const kb_sim *sim, int planes) {
    if (!(planes & KB_GRID_OBJECTS) || sim->cfg.num_objects > 0) return KB_OK;
    return fail(KB_EINVAL, "%s: KB_GRID_OBJECTS asked for, but the handle has no objects", entry);
}

int kb_grid_channels(const kb_sim *sim, int planes) {
    if (!sim) return fail(KB_EINVAL, "kb_grid_channels: NULL handle");
    if (check_grid_planes("kb_grid_channels", planes) != KB_OK || check_grid_objects("kb_grid_channels", sim, planes) != KB_OK) return KB_EINVAL;
    return (planes & KB_GRID_COUNT ? 1 : 0) + (planes & KB_GRID_FLOW ? 2 : 0) + (planes & KB_GRID_OBJECTS ? sim->cfg.num_objects : 0);
}

int kb_sense_grid(kb_sim *sim, int gw, int gh, int planes, float *d_out, void *stream) {
    if (!sim || !d_out) return fail(KB_EINVAL, "kb_sense_grid: NULL argument");
    if (check_grid_planes("kb_sense_grid", planes) != KB_OK) return KB_EINVAL;
    if (gw < 1 || gw > KB_GRID_MAX_SIDE || gh < 1 || gh > KB_GRID_MAX_SIDE) return fail(KB_EINVAL, "kb_sense_grid: 1 <= gw, gh <= KB_GRID_MAX_SIDE (128) required");
    if (check_grid_objects("kb_sense_grid", sim, planes) != KB_OK) return KB_EINVAL;
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_grid: kb_bind() first");
    const Params &p = sim->p;
    const int C = kb_grid_channels(sim, planes), bots = planes & (KB_GRID_COUNT | KB_GRID_FLOW);
    const int words = (bots & KB_GRID_COUNT ? 1 : 0) + (bots & KB_GRID_FLOW ? 2 : 0);
    const float wx = p.xmax - p.xmin, wy = p.ymax - p.ymin;        // (kb_outline.arena is these four)
    if (bots) {
        const GridLds L(gw, gh, words);
        const int vec = gw % 4 == 0 && aligned16(d_out);
        const auto fn = bots == KB_GRID_COUNT ? kb_grid_bots_kernel<KB_GRID_COUNT> : bots == KB_GRID_FLOW ? kb_grid_bots_kernel<KB_GRID_FLOW>
                                                                                   : kb_grid_bots_kernel<KB_GRID_COUNT | KB_GRID_FLOW>;
        const int rc = launch("kb_sense_grid", fn, (unsigned)p.E * (unsigned)L.bands, 256, L.bytes, stream, p.N, gw, gh, L.bands, L.rows, C, vec, p.xmin, p.ymin, (float)gw / wx, (float)gh / wy, p.buf.x, p.buf.y, p.buf.theta, d_out);
        if (rc != KB_OK) return rc;
    }
    if (planes & KB_GRID_OBJECTS) {
        kb_outline ol;
        kb_get_outline(sim, &ol);
        const int cells = gw * gh;
        const int threads = cells < 256 ? (cells + 63) & ~63 : 256;        // one cell per lane: no idle waves in a small grid
        const int tiles = (cells + threads - 1) / threads;
        return launch("kb_sense_grid", kb_grid_objects_kernel, (unsigned)p.E * (unsigned)tiles, threads, ObjectsLds().bytes, stream, ol, gw, gh, tiles, C, words, wx / (float)gw, wy / (float)gh, p.buf.ox, p.buf.oy, p.buf.otheta, d_out);
    }
    return KB_OK;
}

int kb_sense_coverage(kb_sim *sim, int gw, int gh, const uint8_t *d_select, int32_t *d_owner, float *d_dist, float *d_cell, float *d_stats,
                      void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_sense_coverage: NULL handle");
    if (gw < 1 || gw > KB_GRID_MAX_SIDE || gh < 1 || gh > KB_GRID_MAX_SIDE) return fail(KB_EINVAL, "kb_sense_coverage: 1 <= gw, gh <= KB_GRID_MAX_SIDE (128) required");
    if (!d_owner && !d_dist && !d_cell && !d_stats) return fail(KB_EINVAL, "kb_sense_coverage: d_owner, d_dist, d_cell and d_stats are all NULL");
    if (!aligned16(d_cell)) return fail(KB_EINVAL, "kb_sense_coverage: d_cell must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_coverage: kb_bind() first");
    const Params &p = sim->p;
    const CoverageArgs a = {gw, gh, (p.xmax - p.xmin) / (float)gw, (p.ymax - p.ymin) / (float)gh};       // (kb_outline.arena is these four)
    return launch("kb_sense_coverage", kb_coverage_kernel, p.E, 256, CoverageLds(p.NP, p.ncell).bytes, stream, p, a, d_select, d_owner, d_dist, reinterpret_cast<float4 *>(d_cell), d_stats);
}

int kb_field_step(kb_sim *sim, int gw, int gh, int n_channels, const float *keep, const float *spread, int n_iters, const uint8_t *d_env_mask,
                  const float *d_amount, float *d_field, float *d_sense, void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_field_step: NULL handle");
    if (gw < 1 || gw > KB_GRID_MAX_SIDE || gh < 1 || gh > KB_GRID_MAX_SIDE) return fail(KB_EINVAL, "kb_field_step: 1 <= gw, gh <= KB_GRID_MAX_SIDE (128) required");
    if (n_channels < 1 || n_channels > KB_FIELD_MAX_CHANNELS) return fail(KB_EINVAL, "kb_field_step: 1 <= n_channels <= KB_FIELD_MAX_CHANNELS (4) required");
    if (!keep || !spread) return fail(KB_EINVAL, "kb_field_step: keep and spread must not be NULL");
    for (int c = 0; c < n_channels; ++c)       // (a NaN fails both comparisons)
        if (!(keep[c] >= 0.0f && keep[c] <= 1.0f) || !(spread[c] >= 0.0f && spread[c] <= 0.25f))
            return fail(KB_EINVAL, "kb_field_step: keep must lie in [0, 1] and spread in [0, 0.25] for every channel");
    if (n_iters < 0 || n_iters > KB_FIELD_MAX_ITERS) return fail(KB_EINVAL, "kb_field_step: 0 <= n_iters <= KB_FIELD_MAX_ITERS (64) required");
    if (!d_field) return fail(KB_EINVAL, "kb_field_step: d_field is NULL");
    if (!d_amount && !d_sense && n_iters == 0) return fail(KB_EINVAL, "kb_field_step: nothing to do (d_amount and d_sense are NULL and n_iters is 0)");
    if (!aligned16(d_sense)) return fail(KB_EINVAL, "kb_field_step: d_sense must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_field_step: kb_bind() first");
    const Params &p = sim->p;
    FieldArgs a;
    memset(&a, 0, sizeof(a));
    a.N = p.N; a.C = n_channels; a.gw = gw; a.gh = gh; a.iters = n_iters;
    a.xmin = p.xmin; a.ymin = p.ymin;        // (kb_outline.arena is these four)
    a.icw = (float)gw / (p.xmax - p.xmin); a.ich = (float)gh / (p.ymax - p.ymin);
    a.hicw = 0.5f * a.icw; a.hich = 0.5f * a.ich;
    for (int c = 0; c < n_channels; ++c) { a.keep[c] = keep[c]; a.spread[c] = spread[c]; }
    const bool vec = gw % 4 == 0 && aligned16(d_field);
    const kb_field_fn fn = vec ? field_kernel<true>(gw * gh) : field_kernel<false>(gw * gh);
    return launch("kb_field_step", fn, (unsigned)p.E * (unsigned)n_channels, FIELD_THREADS, FieldLds(gw, gh).bytes, stream, a, p.buf.x, p.buf.y, p.buf.theta,
                  d_env_mask, d_amount, d_field, reinterpret_cast<float4 *>(d_sense));
}

// the step costs of kb_sense_paths and the unit vector of its diagonals, from the host constants of kb_sense_grid
static void path_costs(const Params &p, int gw, int gh, PathsArgs &a) {
    const float cw = (p.xmax - p.xmin) / (float)gw, ch = (p.ymax - p.ymin) / (float)gh;      // (kb_outline.arena is these four)
    const float dg = sqrtf(cw * cw + ch * ch);
    const auto q = [](float len) { return (int)rintf(fminf(fmaxf(len * 1024.0f, 1.0f), 65536.0f)); };
    a.cw = cw; a.ch = ch;
    a.qx = q(cw); a.qy = q(ch); a.qd = q(dg);
    a.udx = cw / dg; a.udy = ch / dg;
}

int kb_path_costs(const kb_sim *sim, int gw, int gh, int32_t *out) {
    if (!sim || !out) return fail(KB_EINVAL, "kb_path_costs: NULL argument");
    if (gw < 1 || gw > KB_GRID_MAX_SIDE || gh < 1 || gh > KB_GRID_MAX_SIDE) return fail(KB_EINVAL, "kb_path_costs: 1 <= gw, gh <= KB_GRID_MAX_SIDE (128) required");
    PathsArgs a;
    path_costs(sim->p, gw, gh, a);
    out[0] = a.qx; out[1] = a.qy; out[2] = a.qd;
    return KB_OK;
}

int kb_sense_paths(kb_sim *sim, int gw, int gh, const uint8_t *d_source, const uint8_t *d_blocked, int objects, float clear_m, float *d_dist,
                   int8_t *d_next, float *d_bot, float *d_stats, void *stream) {
    if (!sim || !d_source) return fail(KB_EINVAL, "kb_sense_paths: NULL argument");
    if (gw < 1 || gw > KB_GRID_MAX_SIDE || gh < 1 || gh > KB_GRID_MAX_SIDE) return fail(KB_EINVAL, "kb_sense_paths: 1 <= gw, gh <= KB_GRID_MAX_SIDE (128) required");
    if (objects < 0 || objects >= (1 << sim->cfg.num_objects)) return fail(KB_EINVAL, "kb_sense_paths: objects must be a mask of the handle's objects (0 <= objects < 2^num_objects)");
    if (!(clear_m >= 0.0f) || !std::isfinite(clear_m)) return fail(KB_EINVAL, "kb_sense_paths: clear_m must be finite and not negative");
    if (!d_dist && !d_next && !d_bot && !d_stats) return fail(KB_EINVAL, "kb_sense_paths: d_dist, d_next, d_bot and d_stats are all NULL");
    if (!aligned16(d_bot)) return fail(KB_EINVAL, "kb_sense_paths: d_bot must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_paths: kb_bind() first");
    const Params &p = sim->p;
    PathsArgs a;
    memset(&a, 0, sizeof(a));
    path_costs(p, gw, gh, a);
    a.N = p.N; a.gw = gw; a.gh = gh; a.objects = objects; a.clear = clear_m > 0.0f;
    a.xmin = p.xmin; a.ymin = p.ymin;
    a.icw = (float)gw / (p.xmax - p.xmin); a.ich = (float)gh / (p.ymax - p.ymin);
    const float Cw = clear_m * WORLD_SCALE;
    a.C2 = Cw * Cw;
    kb_outline ol;
    kb_get_outline(sim, &ol);
    const int lds = PathsLds(gw, gh).bytes;
    if (lds > GRID_LDS_LIMIT && sim->paths_attr_fn != reinterpret_cast<const void *>(kb_paths_kernel)) {
        // the attribute belongs to the kernel on the current device: raised to the hardware limit, as for the step kernels, and
        // once per handle like theirs -- it is no stream operation, so a call that is captured into a graph launches only
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kb_paths_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CU);
        if (err != hipSuccess) return fail(KB_EHIP, "kb_sense_paths: hipFuncSetAttribute: %s", hipGetErrorString(err));
        sim->paths_attr_fn = reinterpret_cast<const void *>(kb_paths_kernel);
    }
    return launch("kb_sense_paths", kb_paths_kernel, p.E, PATHS_THREADS, lds, stream, ol, a, p.buf.x, p.buf.y, p.buf.theta, p.buf.ox, p.buf.oy, p.buf.otheta,
                  d_source, d_blocked, d_dist, reinterpret_cast<signed char *>(d_next), reinterpret_cast<float4 *>(d_bot), d_stats);
}

int kb_sense_targets(kb_sim *sim, const float *d_points, int n_targets, int per_env, float tol_m, const uint8_t *d_bot_select,
                     const uint8_t *d_slot_select, int32_t *d_index, float *d_rel, int32_t *d_owner, float *d_dist, float *d_stats, void *stream) {
    if (!sim || !d_points) return fail(KB_EINVAL, "kb_sense_targets: NULL argument");
    if (n_targets < 1 || n_targets > KB_MAX_TARGETS) return fail(KB_EINVAL, "kb_sense_targets: 1 <= n_targets <= KB_MAX_TARGETS (1024) required");
    if (!(tol_m >= 0.0f) || !std::isfinite(tol_m)) return fail(KB_EINVAL, "kb_sense_targets: tol_m must be finite and not negative");
    if (!d_index && !d_rel && !d_owner && !d_dist && !d_stats) return fail(KB_EINVAL, "kb_sense_targets: d_index, d_rel, d_owner, d_dist and d_stats are all NULL");
    if (!aligned16(d_rel)) return fail(KB_EINVAL, "kb_sense_targets: d_rel must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_targets: kb_bind() first");
    const Params &p = sim->p;
    const float Tw = tol_m * WORLD_SCALE;
    const TargetsArgs a = {p.N, n_targets, per_env != 0, Tw * Tw};
    return launch("kb_sense_targets", kb_targets_kernel, p.E, TARGETS_THREADS, TargetsLds(p.N, n_targets).bytes, stream, a, p.buf.x, p.buf.y, p.buf.theta, d_points,
                  d_bot_select, d_slot_select, d_index, reinterpret_cast<float4 *>(d_rel), d_owner, d_dist, d_stats);
}

int kb_sense_assign(kb_sim *sim, const float *d_points, int n_targets, int per_env, float tol_m, float cutoff_m, const uint8_t *d_bot_select,
                    const uint8_t *d_slot_select, int32_t *d_index, float *d_rel, int32_t *d_owner, float *d_dist, float *d_stats, void *stream) {
    if (!sim || !d_points) return fail(KB_EINVAL, "kb_sense_assign: NULL argument");
    if (n_targets < 1 || n_targets > KB_MAX_TARGETS) return fail(KB_EINVAL, "kb_sense_assign: 1 <= n_targets <= KB_MAX_TARGETS (1024) required");
    if (!(tol_m >= 0.0f) || !std::isfinite(tol_m)) return fail(KB_EINVAL, "kb_sense_assign: tol_m must be finite and not negative");
    if (!(cutoff_m >= 0.0f)) return fail(KB_EINVAL, "kb_sense_assign: cutoff_m must be a number and not negative (+inf: no cutoff)");
    if (!d_index && !d_rel && !d_owner && !d_dist && !d_stats) return fail(KB_EINVAL, "kb_sense_assign: d_index, d_rel, d_owner, d_dist and d_stats are all NULL");
    if (!aligned16(d_rel)) return fail(KB_EINVAL, "kb_sense_assign: d_rel must be 16-byte aligned");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_assign: kb_bind() first");
    const Params &p = sim->p;
    const float Tw = tol_m * WORLD_SCALE, Cw = cutoff_m * WORLD_SCALE;
    const AssignArgs a = {p.N, n_targets, per_env != 0, Tw * Tw, Cw * Cw};
    return launch("kb_sense_assign", kb_assign_kernel, p.E, TARGETS_THREADS, AssignLds(p.N, n_targets).bytes, stream, a, p.buf.x, p.buf.y, p.buf.theta, d_points,
                  d_bot_select, d_slot_select, d_index, reinterpret_cast<float4 *>(d_rel), d_owner, d_dist, d_stats);
}

int kb_render_default_style(kb_render_style *out) {
    if (!out) return fail(KB_EINVAL, "kb_render_default_style: NULL argument");
    const uint8_t table[3] = {255, 255, 255}, body[3] = {150, 150, 150}, ring[3] = {100, 100, 100}, mark[3] = {255, 255, 255};
    const uint8_t light[3] = {255, 255, 30}, obj[3] = {93, 133, 195};
    for (int c = 0; c < 3; ++c) {
        out->table[c] = table[c]; out->body[c] = body[c]; out->ring[c] = ring[c]; out->mark[c] = mark[c]; out->light[c] = light[c];
        for (int m = 0; m < KB_MAX_OBJECTS; ++m) out->obj[m][c] = obj[c];
    }
    out->light_alpha = 150;
    return KB_OK;
}

int kb_render(kb_sim *sim, int width, int height, int layers, const kb_render_style *style, const uint32_t *d_body_rgb,
              const uint32_t *d_mark_rgb, uint8_t *d_rgb, void *stream) {
    if (!sim || !d_rgb) return fail(KB_EINVAL, "kb_render: NULL argument");
    if (layers <= 0 || (layers & ~(KB_RENDER_OBJECTS | KB_RENDER_BOTS | KB_RENDER_LIGHT)))
        return fail(KB_EINVAL, "kb_render: layers must be a non-empty subset of KB_RENDER_OBJECTS | KB_RENDER_BOTS | KB_RENDER_LIGHT");
    if (width < 1 || width > KB_RENDER_MAX_SIDE || height < 1 || height > KB_RENDER_MAX_SIDE)
        return fail(KB_EINVAL, "kb_render: 1 <= width, height <= KB_RENDER_MAX_SIDE (2048) required");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_render: kb_bind() first");
    const Params &p = sim->p;
    kb_render_style st;
    if (style) st = *style;
    else kb_render_default_style(&st);
    const auto rgb = [](const uint8_t *c) { return (unsigned)c[0] << 16 | (unsigned)c[1] << 8 | (unsigned)c[2]; };
    RenderArgs a;
    memset(&a, 0, sizeof(a));
    const RenderLds L(p.NP, p.ncell, width, height);
    a.width = width; a.height = height; a.layers = layers; a.bands = L.bands; a.band_rows = L.rows;
    a.cw = (p.xmax - p.xmin) / (float)width; a.ch = (p.ymax - p.ymin) / (float)height;       // (kb_outline.arena is these four)
    const float r = sim->cfg.bot_radius, ro = r + 0.002f, Ro = ro * WORLD_SCALE;
    a.Ro2 = Ro * Ro;
    a.Ri = (ro - 0.005f) * WORLD_SCALE; a.Ri2 = a.Ri * a.Ri;
    a.Lf = (r - 0.005f) * WORLD_SCALE; a.Hw = 0.0025f * WORLD_SCALE;
    const bool positional = sim->cfg.light_type == KB_LIGHT_CIRCULAR || sim->cfg.light_type == KB_LIGHT_MOMENTUM || sim->cfg.light_type == KB_LIGHT_COMPOSITE;
    a.nlights = (layers & KB_RENDER_LIGHT) && positional ? p.lcount : 0;
    for (int l = 0; l < a.nlights; ++l) { const float Rl = p.lradius[l] * WORLD_SCALE; a.Rl2[l] = Rl * Rl; }
    a.table = rgb(st.table); a.body = rgb(st.body); a.ring = rgb(st.ring); a.mark = rgb(st.mark); a.light = rgb(st.light); a.alpha = st.light_alpha;
    for (int m = 0; m < KB_MAX_OBJECTS; ++m) a.obj[m] = rgb(st.obj[m]);
    kb_outline ol;
    kb_get_outline(sim, &ol);
    return launch("kb_render", kb_render_kernel, (unsigned)p.E * (unsigned)L.bands, 256, L.bytes, stream, p, ol, a, reach_cells(p, Ro), d_body_rgb, d_mark_rgb, d_rgb);
}

int kb_sense_contacts(kb_sim *sim, int k, float scale, int32_t *d_partner, float *d_impulse, float *d_touch, float *d_obj, void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_sense_contacts: NULL handle");
    if (!d_partner != !d_impulse) return fail(KB_EINVAL, "kb_sense_contacts: d_partner and d_impulse go together: both or neither");
    if (d_partner && (k < 1 || k > KB_MAX_CONTACT_SLOTS)) return fail(KB_EINVAL, "kb_sense_contacts: 1 <= k <= KB_MAX_CONTACT_SLOTS (16) required");
    if (!(scale > 0.0f && scale < INFINITY)) return fail(KB_EINVAL, "kb_sense_contacts: scale must be finite and positive");
    if (!d_partner && !d_touch && !d_obj) return fail(KB_EINVAL, "kb_sense_contacts: all outputs are NULL");
    if (d_obj && sim->cfg.num_objects == 0) return fail(KB_EINVAL, "kb_sense_contacts: d_obj given, but the handle has no objects");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_sense_contacts: kb_bind() first");
    const Params &p = sim->p;
    ContactsArgs a;
    memset(&a, 0, sizeof(a));
    a.N = p.N; a.M = p.M; a.F = p.F; a.cap = p.cap;
    for (int f = 0; f < p.F; ++f) a.body[f] = ot_body(p.otab[f]);       // (kb_create checked 0 <= body < M)
    const int lists = d_partner != nullptr;
    const int vec = (lists && k % 4 == 0 && aligned16(d_partner, d_impulse) ? 1 : 0) | (aligned16(d_touch) ? 2 : 0);
    const auto fn = !lists ? kb_contacts_kernel<0> : k <= 4 ? kb_contacts_kernel<4> : k <= 8 ? kb_contacts_kernel<8> : kb_contacts_kernel<16>;
    return launch("kb_sense_contacts", fn, p.E, 256, ContactsLds(p.N).bytes, stream, a, k, vec, scale, p.buf.ws_key, p.buf.ws_acc, p.buf.ws_cnt, reinterpret_cast<uint2 *>(p.buf.scratch), d_partner, d_impulse, d_touch, d_obj);
}

int kb_light_sense(kb_sim *sim, const float *d_light_action, void *stream) {
    if (!sim) return fail(KB_EINVAL, "kb_light_sense: NULL handle");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_light_sense: kb_bind() first");
    if (sim->cfg.light_type == KB_LIGHT_NONE) return fail(KB_EINVAL, "kb_light_sense: the handle has no light");
    const Params &p = sim->p;
    if (!p.buf.light_value || !p.buf.light_gx || !p.buf.light_gy) return fail(KB_EINVAL, "kb_light_sense: kb_buffers.light_value / light_gx / light_gy are not bound");
    hipLaunchKernelGGL(kb_light_sense_kernel, dim3((unsigned)p.E), dim3(256), 0, (hipStream_t)stream, p, d_light_action);
    return launched("kb_light_sense");
}

// the spawn launch of kb_reset and kb_reset_envs (d_env_mask NULL: every env, init NULL: nothing but the kilobots' rows)
static int reset_launch(const char *entry, kb_sim *sim, const kb_reset_params *rp, const uint8_t *d_env_mask, const kb_episode_init *init,
                        void *stream) {
    const Params &p = sim->p;
    ResetArgs a;
    a.k0 = (unsigned)(rp->seed & 0xFFFFFFFFull); a.k1 = (unsigned)(rp->seed >> 32);
    a.env_offset = rp->env_offset; a.random_theta = rp->random_theta; a.random_velocity = rp->random_velocity;
    a.mean_x = rp->mean[0]; a.mean_y = rp->mean[1]; a.std = rp->std;
    // world_bounds -/+ 0.02 (yaml_kilobots_env.py:350-351), metres
    a.lo_x = -0.5f * sim->cfg.world_width + 0.02f; a.hi_x = 0.5f * sim->cfg.world_width - 0.02f;
    a.lo_y = -0.5f * sim->cfg.world_height + 0.02f; a.hi_y = 0.5f * sim->cfg.world_height - 0.02f;
    a.env_mask = d_env_mask;
    a.episode = init ? init->d_episode : nullptr;
    a.obj_pose = init ? init->d_obj_pose : nullptr;
    a.light_pos = init ? init->d_light_pos : nullptr;
    a.light_vel = init ? init->d_light_vel : nullptr;
    const size_t T = (size_t)p.E * p.N;
    hipLaunchKernelGGL(kb_reset_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, a);
    return launched(entry);
}

int kb_reset(kb_sim *sim, const kb_reset_params *rp, void *stream) {
    if (!sim || !rp) return fail(KB_EINVAL, "kb_reset: NULL argument");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_reset: kb_bind() first");
    if (!(rp->std >= 0.0f)) return fail(KB_EINVAL, "kb_reset: std must be >= 0");
    const int rc = reset_launch("kb_reset", sim, rp, nullptr, nullptr, stream);
    if (rc != KB_OK) return rc;
    if (rp->resolve) return kb_step(sim, nullptr, nullptr, 1, KB_STEP_NO_DRIVE, stream);
    return KB_OK;
}

int kb_reset_envs(kb_sim *sim, const kb_reset_params *rp, const uint8_t *d_env_mask, const kb_episode_init *init, void *stream) {
    if (!sim || !rp || !d_env_mask) return fail(KB_EINVAL, "kb_reset_envs: NULL argument");
    if (!(rp->std >= 0.0f)) return fail(KB_EINVAL, "kb_reset_envs: std must be >= 0");
    if (init && init->d_obj_pose && sim->cfg.num_objects == 0) return fail(KB_EINVAL, "kb_reset_envs: d_obj_pose, but the handle has no objects");
    if (init && (init->d_light_pos || init->d_light_vel) && sim->cfg.light_type == KB_LIGHT_NONE)
        return fail(KB_EINVAL, "kb_reset_envs: d_light_pos / d_light_vel, but the handle has no light");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_reset_envs: kb_bind() first");
    const int rc = reset_launch("kb_reset_envs", sim, rp, d_env_mask, init, stream);
    if (rc != KB_OK) return rc;
    if (rp->resolve) return step_launch("kb_reset_envs", sim, d_env_mask, nullptr, nullptr, 1, KB_STEP_NO_DRIVE, stream);
    return KB_OK;
}

int kb_get_poses(kb_sim *sim, float *d_out, void *stream) {
    if (!sim || !d_out) return fail(KB_EINVAL, "kb_get_poses: NULL argument");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_get_poses: kb_bind() first");
    const size_t T = (size_t)sim->p.E * sim->p.N;
    hipLaunchKernelGGL(kb_get_poses_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       sim->p.buf.x, sim->p.buf.y, sim->p.buf.theta, d_out, T);
    return launched("kb_get_poses");
}

int kb_get_state(kb_sim *sim, float *d_out, void *stream) {
    if (!sim || !d_out) return fail(KB_EINVAL, "kb_get_state: NULL argument");
    if (!sim->bound) return fail(KB_ENOTBOUND, "kb_get_state: kb_bind() first");
    const size_t T = (size_t)sim->p.E * (size_t)(sim->p.N + sim->p.M + 1);
    hipLaunchKernelGGL(kb_get_state_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sim->p, d_out);
    return launched("kb_get_state");
}

int kb_lds_bytes(const kb_sim *sim) { return sim ? sim->p.lds_total : KB_EINVAL; }
int kb_light_action_dim(const kb_sim *sim) { return sim ? sim->p.ladim : KB_EINVAL; }
int kb_light_count(const kb_sim *sim) { return sim ? (sim->cfg.light_type == KB_LIGHT_NONE ? 0 : sim->p.lcount) : KB_EINVAL; }
// per contact: the 16-byte staging record + the 16-byte level-sorted record (pair, normal, impulse) of the cooperative sweeps (kernels with objects: normal and effective mass, 12 B)
size_t kb_scratch_bytes(const kb_sim *sim) { return sim ? (size_t)sim->p.E * (size_t)sim->p.cap * 32u : 0; }
int kb_exact_division(const kb_sim *sim) { return sim ? sim->p.exact_div : KB_EINVAL; }

int kb_exact_selftest(const kb_sim *sim, unsigned long long *d_counts, void *stream) {
    if (!sim || !d_counts) return fail(KB_EINVAL, "kb_exact_selftest: NULL argument");
    const float kbb = sim->p.im_bot + sim->p.im_bot, kwb = 0.0f + sim->p.im_bot;
    if (hipMemsetAsync(d_counts, 0, 6 * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess) return launched("kb_exact_selftest");
    hipLaunchKernelGGL(kb_exact_selftest_kernel, dim3(1u << 16), dim3(256), 0, (hipStream_t)stream, kbb, kwb, d_counts);
    return launched("kb_exact_selftest");
}

int kb_debug_lds(int mode, uint32_t word, unsigned long long *d_count, void *stream) {
    if (mode != 0 && mode != 1) return fail(KB_EINVAL, "kb_debug_lds: mode must be 0 (fill) or 1 (count)");
    if (mode == 1 && !d_count) return fail(KB_EINVAL, "kb_debug_lds: mode 1 needs d_count");
    int device = 0, cus = 0;
    hipError_t err = hipGetDevice(&device);
    if (err == hipSuccess) err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (err == hipSuccess) err = hipFuncSetAttribute(reinterpret_cast<const void *>(kb_debug_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CU);
    if (err != hipSuccess || cus <= 0) return fail(KB_EHIP, "kb_debug_lds: %s", hipGetErrorString(err));
    if (mode == 1 && hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess) return launched("kb_debug_lds");
    hipLaunchKernelGGL(kb_debug_lds_kernel, dim3(2u * (unsigned)cus), dim3(DEBUG_LDS_THREADS), (size_t)LDS_CU, (hipStream_t)stream, mode, (unsigned)word, d_count);
    return launched("kb_debug_lds");
}

int kb_contact_capacity(const kb_sim *sim) { return sim ? sim->p.cap : KB_EINVAL; }
int kb_lds_staging_entries(const kb_sim *sim) { return sim ? sim->p.capL : KB_EINVAL; }
int kb_block_threads(const kb_sim *sim) { return sim ? sim->threads : KB_EINVAL; }
int kb_variant_index(const kb_sim *sim) { return sim ? sim->variant : -1; }
int kb_set_block_threads(kb_sim *sim, int threads) {
    if (!sim || threads == 0) return fail(KB_EINVAL, "kb_set_block_threads: multiple of 64 up to the build maximum");   // (0: plan_launch would choose)
    const Plan pl = plan_launch(plan_input(sim, threads));
    if (pl.status != KB_OK) return fail(pl.status, "%s", pl.msg);
    use_plan(sim, pl);
    return KB_OK;
}

}  // extern "C"
